"""The regime table of tests/launch_regimes.py against the plans the library computes (fldbg_launch_plans: host arithmetic, no GPU).

If a threshold of a plan moves, these tests name the regime whose grid no longer reaches its branch: the -m gpu modules
tests/test_gpu_launch_regimes.py, tests/test_gpu_momentum_regimes.py, tests/test_gpu_mg_regimes.py and tests/test_gpu_rank_regimes.py then check another plan
than the one they were written for, and the table must be re-aimed."""
import pytest

from tests.launch_regimes import (BY_NAME, CAVITY, CHANNEL, FIELDS, PER, PRODUCTION, PRODUCTION_MG, RANK_REGIMES, REGIMES, SYM, TOY_RANK_BLOCKS, XPER, O, V,
                                  launch_plans, mg_levels, mg_plans, mg_restrict_fused, mg_summary, mom_last_chunk, mom_regime, mom_tiles, six_trips)


@pytest.mark.parametrize("reg", REGIMES, ids=[r.name for r in REGIMES])
def test_regime_grid_takes_its_plan(reg):
    got = launch_plans(reg.n)
    wrong = {k: (v, got[k]) for k, v in reg.expect.items() if got[k] != v}
    assert not wrong, f"regime {reg.name} {reg.n} left its plan ({reg.reaches}); field: (expected, got) {wrong}"


def test_table_covers_every_branch():
    plans = {r.name: launch_plans(r.n) for r in REGIMES}
    # plan_cg_A: the two small rules, the 8-wave standard tiles and the mid rule
    assert {p["cg.regime"] for p in plans.values()} >= {"small", "small_ry1", "standard", "mid"}
    for name in ("cg_standard_ragged", "cg_mid_ragged"):
        p, (nx, ny, nz) = plans[name], BY_NAME[name].n
        assert p["cg.nw"] == 8
        assert nx % 128 != 0 and ny % (p["cg.nw"] * p["cg.ry"]) != 0, f"{name}: the last 8-wave tile is full in x or y"
        assert p["cg.nchunk"] > 1 and nz % p["cg.zc"] != 0, f"{name}: no ragged z chunk seam"
        assert six_trips(p) > 1, f"{name}: k_project_six takes one grid-stride trip"
    # fl_cheb2_plan: the clamp, once with several z chunks (a ragged seam)
    assert any(p["cheb2.clamp"] and p["cheb2.nchunk"] > 1 and BY_NAME[k].n[2] % p["cheb2.zc"] != 0 for k, p in plans.items())
    # k_schur_var: the full 128 blocks per XCD, with and without a fixed x segment, a short last y band
    s = [(p["schur.per_xcd"], p["schur.fixed_seg"]) for p in plans.values()]
    assert (128, 1) in s and (128, 0) in s
    assert any(p["schur.fixed_seg"] and BY_NAME[k].n[1] % p["schur.band"] != 0 for k, p in plans.items())
    # and the boundary types: a null space, the channel's periodic z seam over several chunks, a periodic x seam on a partial tile
    from tests.launch_regimes import CAVITY, CHANNEL, XPER
    bcs = [(r.name, bc) for r in REGIMES for bc in r.bcs]
    assert any(bc == CHANNEL and plans[n]["cg.nchunk"] > 1 for n, bc in bcs)
    assert any(bc == XPER and BY_NAME[n].n[0] % 128 != 0 and plans[n]["cg.nw"] == 8 for n, bc in bcs)
    assert any(bc == CAVITY for _, bc in bcs)


def test_table_covers_every_branch_of_the_momentum_tiling():
    """the t2 tiling of k_mom3 / k_mom2 / k_mom_pw3 (fl_momentum_create): both bounds of the chunk count, the seams and ragged edges a tile walk
    gets wrong, and the block order with and without the XCD remap"""
    from tests.launch_regimes import CHANNEL
    mom = {r.name: (r, launch_plans(r.n)) for r in REGIMES if any(k.startswith("mom.") for k in r.expect)}
    # the chunk count comes from the bound mom_regime names: about 1024 blocks over the tiles, or chunks of at least 8 planes
    for name, (r, p) in mom.items():
        nz, reg, tiles = r.n[2], mom_regime(p, r.n), mom_tiles(p, r.n)
        nc = min((1024 + tiles // 2) // tiles if reg == "tile" else max(1, nz // 8), nz)
        assert p["mom.t2zc"] == -(-nz // nc) and p["mom.t2blocks"] == tiles * p["mom.t2chunk"], \
            f"{name} {r.n}: the t2 chunks no longer follow the {reg} bound ({r.reaches}): {nc} chunks wanted, got {p['mom.t2chunk']} of {p['mom.t2zc']}"
    assert {mom_regime(p, r.n) for r, p in mom.values()} == {"tile", "nz"}
    assert all(mom_regime(launch_plans(n), n) == "tile" for n in PRODUCTION)        # what 256^3 - 512^3 take
    covered = {
        # long chunks like 256^3 - 512^3, the last one shorter
        "t2zc >= 32, short last chunk": [k for k, (r, p) in mom.items() if p["mom.t2zc"] >= 32 and mom_last_chunk(p, r.n) < p["mom.t2zc"]],
        # a last chunk of one plane: the pipeline's k+1 / k+2 planes are both past the chunk, for k_mom3 (ny > 8) and for k_mom2 (ny <= 8)
        "last chunk of one plane, ny > 8": [k for k, (r, p) in mom.items() if p["mom.t2chunk"] > 1 and mom_last_chunk(p, r.n) == 1 and r.n[1] > 8],
        "last chunk of one plane, ny <= 8": [k for k, (r, p) in mom.items() if p["mom.t2chunk"] > 1 and mom_last_chunk(p, r.n) == 1 and r.n[1] <= 8],
        # xcd_remap (flags & 1) on and off, each over several chunks
        "XCD remap, several chunks": [k for k, (r, p) in mom.items() if p["mom.t2blocks"] % 8 == 0 and p["mom.t2chunk"] > 1],
        "no XCD remap, several chunks": [k for k, (r, p) in mom.items() if p["mom.t2blocks"] % 8 != 0 and p["mom.t2chunk"] > 1],
        # a full last x tile (16-byte pair stores) and a last x tile of one odd column
        "nx % 128 == 0": [k for k, (r, p) in mom.items() if r.n[0] % 128 == 0],
        "last x tile of 1 column": [k for k, (r, p) in mom.items() if r.n[0] % 128 == 1 and p["mom.t2x"] > 1],
        "last y tile of 1 row, ny > 8": [k for k, (r, p) in mom.items() if r.n[1] % 8 == 1 and r.n[1] > 8],
        # the periodic z seam of the channel across several chunks
        "CHANNEL, several chunks": [k for k, (r, p) in mom.items() if CHANNEL in r.bcs and p["mom.t2chunk"] > 1],
    }
    missing = [what for what, names in covered.items() if not names]
    assert not missing, f"no momentum regime reaches: {missing}"


@pytest.mark.parametrize("reg", RANK_REGIMES, ids=[r.name for r in RANK_REGIMES])
def test_rank_regime_blocks_take_their_plans(reg):
    """every rank's block, formed as the library forms it (fl_decomp_default / the ownership ranges), has the table's shape and takes the table's plan"""
    size = reg.ranks[0] * reg.ranks[1] * reg.ranks[2]
    cells = 0
    for rank in range(size):
        d = reg.decomp(rank)
        blk = tuple(int(d.len[a]) for a in range(3))
        assert blk == reg.blocks[rank], f"regime {reg.name}: rank {rank} owns {blk}, the table says {reg.blocks[rank]}"
        cells += blk[0] * blk[1] * blk[2]
        got = launch_plans(blk)
        wrong = {k: (v, got[k]) for k, v in reg.expect[rank].items() if got[k] != v}
        assert not wrong, f"regime {reg.name} {reg.n}, rank {rank} block {blk} left its plan ({reg.reaches}); field: (expected, got) {wrong}"
    assert cells == reg.n[0] * reg.n[1] * reg.n[2], f"regime {reg.name}: the blocks do not tile the grid"


def test_rank_table_covers_every_edge_of_the_several_rank_path():
    """what tests/test_gpu_rank_regimes.py is there for: rank faces, periodic seams, two-hop edges and ragged block edges on 8-wave plans, the
    clamped k_cheb2 plan over several chunks, k_schur_var_ring at 128 blocks per XCD -- and that the toy grids of the other several-rank tests
    reach none of the 8-wave plans"""
    plans = {r.name: [launch_plans(b) for b in r.blocks] for r in RANK_REGIMES}
    w8 = [r for r in RANK_REGIMES if all(p["cg.nw"] == 8 for p in plans[r.name])]
    left = [(r.name, b) for r in RANK_REGIMES if not r.name.startswith("ranks_schur") for b, p in zip(r.blocks, plans[r.name]) if p["cg.nw"] != 8]
    assert not left, f"blocks that left the 8-wave plans: {left}"
    regime = lambda r: {p["cg.regime"] for p in plans[r.name]}
    blocks8 = [(r, b, p) for r in w8 for b, p in zip(r.blocks, plans[r.name])]
    covered = {
        # a rank face on every axis in the standard regime, on x and y in the mid regime
        **{f"standard, rank face on axis {a}": [r.name for r in w8 if regime(r) == {"standard"} and r.ranks[a] > 1] for a in range(3)},
        **{f"mid, rank face on axis {a}": [r.name for r in w8 if regime(r) == {"mid"} and r.ranks[a] > 1] for a in range(2)},
        # a periodic axis split over two ranks (the same peer on both sides), and one held by one rank (wrap_local) next to a split axis
        "periodic axis over two ranks": [r.name for r in w8 for bc in r.bcs for a in range(3) if r.periodic(bc)[a] and r.ranks[a] == 2],
        "periodic axis inside the block next to a split axis": [r.name for r in w8 for bc in r.bcs for a in range(3)
                                                                if r.periodic(bc)[a] and r.ranks[a] == 1 and max(r.ranks) > 1],
        # three ranks on an axis: the middle block has two different peers (and, on a non-periodic axis, no wall row)
        "an interior block": [r.name for r in w8 if max(r.ranks) >= 3],
        # 2 x 2 ranks: the edge cells of fl_fill_ghosts_deep travel in two hops
        "2 x 2 rank grid": [r.name for r in w8 if sorted(r.ranks) == [1, 2, 2]],
        # ragged block edges: odd nx / ny (the last cell / row alone in its pair), partial last tiles, a short last z chunk
        "odd nx": [r.name for r, b, p in blocks8 if b[0] % 2 == 1],
        "odd ny": [r.name for r, b, p in blocks8 if b[1] % 2 == 1],
        "cheb2 clamp, several z chunks": [r.name for r, b, p in blocks8 if p["cheb2.clamp"] == 1 and p["cheb2.nchunk"] > 1 and b[2] % p["cheb2.zc"] != 0],
        # k_schur_var_ring: the full launch, with and without a fixed x segment; a split of each axis
        "schur ring, fixed segment": [r.name for r in RANK_REGIMES if all(p["schur.per_xcd"] == 128 and p["schur.fixed_seg"] == 1 for p in plans[r.name])
                                      and r.name.startswith("ranks_schur")],
        "schur ring, general segments": [r.name for r in RANK_REGIMES if all(p["schur.per_xcd"] == 128 and p["schur.fixed_seg"] == 0 for p in plans[r.name])
                                         and r.name.startswith("ranks_schur")],
        **{f"schur ring, split of axis {a}": [r.name for r in RANK_REGIMES if r.name.startswith("ranks_schur") and r.ranks[a] == 2] for a in range(3)},
    }
    missing = [what for what, names in covered.items() if not names]
    assert not missing, f"no rank regime reaches: {missing}"
    assert {tuple(bc) for r in w8 for bc in r.bcs} >= {tuple(CAVITY), tuple(CHANNEL), tuple(XPER)}
    for r, b, p in blocks8:
        assert b[0] % 128 != 0 and b[1] % 16 != 0, f"{r.name} {b}: the last 8-wave tile is full in x or y"
        assert p["cg.nchunk"] > 1 and b[2] % p["cg.zc"] != 0, f"{r.name} {b}: no short last z chunk"
        assert six_trips(p) > 1, f"{r.name} {b}: k_project_six takes one grid-stride trip"
    for r in RANK_REGIMES:
        if r.name.startswith("ranks_schur"):
            assert all(p["schur.per_xcd"] == 128 for p in plans[r.name]), r.name
    # the several-rank tests on toy grids: no block of theirs takes an 8-wave plan
    for b in TOY_RANK_BLOCKS:
        assert launch_plans(b)["cg.nw"] != 8, b


MOM = [r for r in REGIMES if r.name.startswith("mom_")]


@pytest.mark.parametrize("reg", MOM, ids=[r.name for r in MOM])
def test_momentum_regime_grid_tells_its_columns_rows_and_planes_apart(reg):
    """tests/test_gpu_momentum_regimes.py runs the momentum regimes stretched in all three axes.  There the 1-D rows of a cell -- the viscous row
    and the B rows of its low face -- differ from those of the cell a tiling slip would read instead (the next one; one x tile, y tile or z chunk
    further) by far more than the parity tolerance of 2e-13: a kernel that takes the numbers of the wrong column, row or plane fails there.  On
    the uniform grid the same slip reads the same numbers."""
    import numpy as np

    from oracle import fluca_oracle as fo
    from tests.gpu_common import CAVITY_BOX, stretched_faces

    def rows(g, d, c):
        """[cell][offset -2..2] of the viscous rows and [cell][offset -2..1] of the B rows of the cells' low faces"""
        lap, b = np.zeros((g.n[d], 5)), np.zeros((g.n[d], 4))
        for i in range(g.n[d]):
            for off, v in g.lap_row(d, i, c):
                lap[i, off + 2] += v
            for col, v in g.B_row(d, i, c):
                b[i, col - i + 2] += v
        return lap, b

    def gap(r, s):
        """per cell pair (i, i + s): how far apart their numbers are, relative to the largest of their kind"""
        return np.max([np.abs(a[s:] - a[:-s]).max(axis=1) / np.abs(a).max() for a in r], axis=0)

    p = launch_plans(reg.n)
    for bc in reg.bcs:
        grids = {"stretched": fo.Grid(reg.n, stretched_faces(reg.n), bc), "uniform": fo.Grid.uniform(reg.n, CAVITY_BOX, bc)}
        for d, tile in enumerate((128, 8, p["mom.t2zc"])):
            n = reg.n[d]
            for c in range(3):
                R = {k: rows(g, d, c) for k, g in grids.items()}
                for s in {1, tile}:
                    if s >= n:
                        continue
                    apart = gap(R["stretched"], s).min()
                    assert apart >= 1e-7, (reg.name, bc, d, c, s, apart)
                    if n - s >= 3:      # two inner cells that far apart: the uniform grid gives them the same numbers
                        assert gap(R["uniform"], s)[1:-1].min() <= 1e-14, (reg.name, bc, d, c, s)


MG = [r for r in REGIMES if r.mg]


@pytest.mark.parametrize("reg", MG, ids=[r.name for r in MG])
def test_multigrid_regime_grid_takes_its_levels(reg):
    """the hierarchy of the regime, level by level: shape, ratio, the plans of the residual + restriction, prolongation, smoother and coarse solve"""
    got = mg_plans(reg.n)
    assert [lv["n"] for lv in got] == [lv["n"] for lv in reg.mg], f"regime {reg.name}: the hierarchy changed ({reg.reaches})"
    wrong = {(l, k): (v, got[l].get(k)) for l, want in enumerate(reg.mg) for k, v in want.items() if got[l].get(k) != v}
    assert not wrong, f"regime {reg.name} {reg.n} left its plans ({reg.reaches}); (level, field): (expected, got) {wrong}"


def test_table_covers_every_branch_of_the_multigrid_cycle():
    """the edges of the cycle at 256^3 - 512^3 that the toy grids of tests/test_gpu_mg.py never reach (all their levels take the small_ry1 plan)"""
    levels = [(r, l, lv) for r in MG for l, lv in enumerate(mg_plans(r.n))]
    inner = [(r, l, lv) for r, l, lv in levels if lv["ratio"] is not None]
    covered = {
        # k_bcgs_st MODE 11 as <2, 8, 11> and <2, 4, 11>, and the two-pass fallback on a level of 8-wave tiles
        "one-pass residual + restriction, 8 waves": [r.name for r, l, lv in inner if lv["rr"] == "fused" and lv["cg.nw"] == 8],
        "one-pass residual + restriction, 4 waves": [r.name for r, l, lv in inner if lv["rr"] == "fused" and lv["cg.nw"] == 4],
        "fallback on an 8-wave level": [r.name for r, l, lv in inner if lv["rr"] == "fallback" and lv["cg.nw"] == 8],
        # k_mg_prolong_lin_cc: three or more 62-column blocks, the last partial; a last z chunk shorter than 4
        "lin_cc, >= 3 x blocks, partial last": [r.name for r, l, lv in inner if lv["prolong"] == "cc" and len(lv["prolong.xblocks"]) >= 3
                                                and lv["prolong.xblocks"][-1] < 62],
        "lin_cc, short last z chunk": [r.name for r, l, lv in inner if lv["prolong"] == "cc" and lv["prolong.zchunks"][-1] < 4
                                       and len(lv["prolong.zchunks"]) > 1],
        # k_mg_prolong_lin_tile<false>: three x tiles and a last z chunk of one plane
        "lin_tile<false>, 3 x tiles": [r.name for r, l, lv in inner if lv["prolong"] == "tile" and len(lv["prolong.xblocks"]) >= 3],
        "lin_tile<false>, last z chunk of one plane": [r.name for r, l, lv in inner if lv["prolong"] == "tile" and lv["prolong.zchunks"][-1] == 1
                                                       and len(lv["prolong.zchunks"]) > 1],
        # the grid-stride kernels take several trips: k_mg_restrict, and k_mg_pwd / k_mg_dots on level 0
        "k_mg_restrict, several trips": [r.name for r, l, lv in inner if lv["rr"] == "fallback" and lv["restrict_trips"] > 2],
        "k_mg_pwd / k_mg_dots, several trips": [r.name for r, l, lv in levels if l == 0 and lv["pw_trips"] > 2],
        # the three fused smoothing steps from zero on 8-wave tiles with several z chunks
        "fused smoother, 8 waves, several z chunks": [r.name for r, l, lv in levels if lv["smoother"] == "fused" and lv["cg.nw"] == 8
                                                      and launch_plans(lv["n"])["cheb2.nchunk"] > 1],
        # both coarse solves
        "k_mg_coarse_cg": [r.name for r, l, lv in levels if lv.get("coarse") == "coarse_cg"],
        "the public Jacobi-PCG as coarse solve": [r.name for r, l, lv in levels if lv.get("coarse") == "pcg"],
    }
    missing = [what for what, names in covered.items() if not names]
    assert not missing, f"no multigrid regime reaches: {missing}"
    # and the toy grids reach none of the one-pass kernel
    for n in ((32, 32, 16), (32, 16, 16), (24, 20, 16), (32, 24, 16), (64, 64, 32)):
        assert all(lv.get("rr") != "fused" for lv in mg_plans(n)), n


@pytest.mark.parametrize("n,bc", [
    ((32, 32, 16), CAVITY), ((32, 16, 16), [PER] * 6), ((24, 20, 16), CHANNEL), ((64, 64, 32), CAVITY), ((15, 15, 15), CAVITY),
    ((40, 24, 16), [O, V, V, V, V, V]), ((64, 32, 32), [PER, PER, V, V, SYM, V]), ((160, 40, 36), CAVITY), ((130, 18, 34), [V, V, PER, PER, SYM, V]),
    ((34, 10, 12), CAVITY),
])
def test_mg_levels_follow_the_oracle(n, bc):
    """mg_levels restates mg_build_levels' rule; the oracle's MgOracle builds its hierarchy by the same rule (the grids of tests/test_gpu_mg.py)"""
    from oracle import fluca_oracle as fo
    g = fo.Grid.uniform(n, [(0.0, 1.0), (0.0, 1.0), (0.0, 0.5)], bc, 1e-3)
    assert mg_levels(n) == [gl.n for gl in fo.MgOracle(g).grids]


@pytest.mark.parametrize("n", list(PRODUCTION_MG), ids=["x".join(map(str, n)) for n in PRODUCTION_MG])
def test_production_shapes_build_their_hierarchy(n):
    got = mg_summary(n)
    want = PRODUCTION_MG[n]
    wrong = {k: (v, got[k]) for k, v in want.items() if got[k] != v}
    assert not wrong, f"production shape {n}: multigrid hierarchy moved; field: (expected, got) {wrong}"


def test_restrict_query_restates_the_launcher():
    """fldbg_mg_restrict_fused against the shape test of fl_residual_restrict_padded, restated from the fields of plan_cg_A: two rows per wave,
    4- or 8-wave tiles, even z chunks, an even block; out-of-range sizes are refused"""
    from fluca_amd import capi
    shapes = [r.n for r in REGIMES] + list(PRODUCTION) + [lv["n"] for r in MG for lv in mg_plans(r.n)]
    shapes += [(a, b, c) for a in (2, 8, 62, 130, 256) for b in (6, 8, 16, 32, 34, 200) for c in (1, 4, 14, 15, 28, 30)]
    for n in shapes:
        p = launch_plans(n)
        want = int(p["cg.ry"] == 2 and p["cg.nw"] in (4, 8) and (p["cg.nchunk"] == 1 or p["cg.zc"] % 2 == 0) and all(m % 2 == 0 for m in n))
        assert mg_restrict_fused(n) == want, (n, p)
    assert {mg_restrict_fused(n) for n in shapes} == {0, 1}
    assert capi.lib.fldbg_mg_restrict_fused(0, 4, 4) < 0 and capi.lib.fldbg_mg_restrict_fused(4, 4, -1) < 0


@pytest.mark.parametrize("n", list(PRODUCTION), ids=["x".join(map(str, n)) for n in PRODUCTION])
def test_production_shapes_map(n):
    got = launch_plans(n)
    want = PRODUCTION[n]
    wrong = {k: (v, got[k]) for k, v in want.items() if got[k] != v}
    assert not wrong, f"production shape {n}: plan moved; field: (expected, got) {wrong}"


def test_plan_query_is_consistent():
    """the fields hold together: blocks = tiles x chunks, the chunks cover z, and out-of-range sizes are refused"""
    from fluca_amd import capi
    for n in [r.n for r in REGIMES] + list(PRODUCTION) + [(1, 1, 1), (6, 5, 4), (130, 37, 20), (64, 64, 32)]:
        p = launch_plans(n)
        assert len(p) == len(FIELDS) + 2
        assert p["cg.nblocks"] == p["cg.tiles_x"] * p["cg.tiles_y"] * p["cg.nchunk"]
        assert (p["cg.nchunk"] - 1) * p["cg.zc"] < n[2] <= p["cg.nchunk"] * p["cg.zc"]
        assert p["cheb2.nblocks"] == p["cheb2.tiles"] * p["cheb2.nchunk"]
        assert (p["cheb2.nchunk"] - 1) * p["cheb2.zc"] < n[2] <= p["cheb2.nchunk"] * p["cheb2.zc"]
        assert (p["tile.nchunk"] - 1) * p["tile.zc"] < n[2] <= p["tile.nchunk"] * p["tile.zc"]
        assert (p["mom.t2chunk"] - 1) * p["mom.t2zc"] < n[2] <= p["mom.t2chunk"] * p["mom.t2zc"]
        assert p["six.nbx"] % p["six.nseg"] == 0 and p["schur.items"] == p["schur.nseg"] * n[1] * n[2]
    assert capi.lib.fldbg_launch_plans(0, 4, 4, None, 0) != 0 and capi.lib.fldbg_launch_plans(4, 4, 4, None, 0) == len(FIELDS)
