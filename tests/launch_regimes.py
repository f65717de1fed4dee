"""The launch shapes of the hot kernels, named: which plan each kernel takes on a grid (fldbg_launch_plans in fl_api.hip, host arithmetic of
the launchers) and the grids of the -m gpu regime tests that reach each one.

The kernels pick their tiling, z chunks and grid stride from the grid size, and the toy grids of the parity suite all land in the small plans.
REGIMES names a grid per plan branch that the product runs at 256^3 - 512^3, made ragged on purpose (partial tiles, a short last z chunk, a
grid stride that wraps), with the fields of the plans it must get; the multigrid regimes name, per level of the hierarchy, the plans of the cycle
(mg_plans).  tests/test_launch_regimes.py checks the table against the library on the CPU; tests/test_gpu_launch_regimes.py,
tests/test_gpu_momentum_regimes.py and tests/test_gpu_mg_regimes.py check every kernel on these grids against the oracle.  RANK_REGIMES names
rank grids whose blocks take the same 8-wave plans (and k_schur_var_ring's 128 blocks per XCD); tests/test_gpu_rank_regimes.py runs the several-rank
kernels on them.  ranks_std_z3 is the one among them with an interior block: three ranks along z, so the middle block keeps q on its first and
its last plane for two different peers (tests/interior_ranks.py has the toy grids with interior ranks)."""
import ctypes as C

from oracle import fluca_oracle as fo

V, O, PER, SYM = fo.BC_VELOCITY, fo.BC_PRESSURE_OUTLET, fo.BC_PERIODIC, fo.BC_SYMMETRY
CAVITY = [V, V, V, V, SYM, V]            # null space
CHANNEL = [V, O, V, V, PER, PER]         # outlet; the periodic z seam crosses the z chunks
XPER = [PER, PER, V, V, PER, PER]        # the periodic x seam joins the partial last tile to tile 0
SLAB = [PER, PER, V, V, O, SYM]          # periodic x, walls in y, an outlet and a symmetry plane at the two z ends

# fldbg_launch_plans' output, in order: <kernel>.<field>
FIELDS = ["cg.ry", "cg.nw", "cg.tiles_x", "cg.tiles_y", "cg.nchunk", "cg.zc", "cg.nblocks",
          "cheb2.nw", "cheb2.tiles_x", "cheb2.tiles", "cheb2.nchunk", "cheb2.zc", "cheb2.nblocks",
          "tile.ry", "tile.tiles_x", "tile.nchunk", "tile.zc", "tile.nblocks",
          "six.nxcd", "six.nseg", "six.nbx", "six.items",
          "schur.per_xcd", "schur.nseg", "schur.band", "schur.fixed_seg", "schur.items",
          "mom.t2x", "mom.t2chunk", "mom.t2zc", "mom.t2blocks"]


def cg_regime(p):
    """the branch of plan_cg_A a plan comes from, read off its shape: one row per wave (small_ry1), 4-wave tiles (small), 8-wave tiles that
    alone nearly fill the chip (standard: >= 128 of them), or fewer 8-wave tiles in several z chunks (mid: >= 2^24 cells)"""
    if p["cg.ry"] == 1:
        return "small_ry1"
    if p["cg.nw"] == 4:
        return "small"
    return "standard" if p["cg.tiles_x"] * p["cg.tiles_y"] >= 128 else "mid"


def cheb2_clamped(p):
    """fl_cheb2_plan's "never a second round of blocks" fired: the nearest chunk count to one wave of 256 blocks would have made more"""
    t = p["cheb2.tiles"]
    return int(t <= 256 and t * max(1, (256 + t // 2) // t) > 256)


def launch_plans(n):
    """{<kernel>.<field>: value} of the plans on an n[0] x n[1] x n[2] block; host arithmetic only (no GPU, no handle)"""
    from fluca_amd import capi
    f = capi.lib.fldbg_launch_plans
    f.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int]
    f.restype = C.c_int
    m = f(*n, None, 0)
    assert m == len(FIELDS), (m, len(FIELDS))
    out = (C.c_int * m)()
    assert f(*n, out, m) == m
    d = dict(zip(FIELDS, out))
    d["cg.regime"] = cg_regime(d)
    d["cheb2.clamp"] = cheb2_clamped(d)
    return d


def six_trips(p):
    """grid-stride trips of the busiest wave of k_project_six (four waves per block)"""
    return -(-p["six.items"] // (4 * p["six.nbx"]))


def mom_tiles(p, n):
    """128 x 8 tiles of the t2 tiling (k_mom3, k_mom2, k_mom_pw3) on an n block"""
    return p["mom.t2x"] * -(-n[1] // 8)


def mom_regime(p, n):
    """the bound that set the z chunk count of the t2 tiling (fl_momentum_create): about 1024 blocks over the tiles ("tile", what 256^3 - 512^3 take:
    long chunks) or chunks of at least 8 planes ("nz", what the toy grids of the parity suite take)"""
    tiles = mom_tiles(p, n)
    return "tile" if (1024 + tiles // 2) // tiles < max(1, n[2] // 8) else "nz"


def mom_last_chunk(p, n):
    """planes of the last z chunk of the t2 tiling"""
    return n[2] - (p["mom.t2chunk"] - 1) * p["mom.t2zc"]


# ---- the multigrid cycle of FL_PC_MG (fl_mg.hip) on one rank
MG_BLOCKS = 4096          # the grid of k_mg_restrict, k_mg_pwd and k_mg_dots is capped at this many 256-thread blocks (nblk)
MG_COARSE_MAX = 4096      # a coarsest level of at most this many cells is solved by one workgroup (k_mg_coarse_cg), else by the public Jacobi-PCG
CHEB2_MIN_CELLS = 32768   # fl_cheb2_agree: a level of at least this many cells smooths with the fused kernel (k_cheb2; cheb_fuse = 1)


def mg_restrict_fused(n):
    """fldbg_mg_restrict_fused (fl_api.hip, host arithmetic): 1 when a level of n cells, halved on every axis, forms the coarse right-hand side
    with the one-pass residual + restriction (k_bcgs_st MODE 11), 0 when it runs the residual and k_mg_restrict"""
    from fluca_amd import capi
    f = capi.lib.fldbg_mg_restrict_fused
    f.argtypes = [C.c_int, C.c_int, C.c_int]
    f.restype = C.c_int
    r = f(*n)
    assert r in (0, 1), (n, r)
    return r


def mg_levels(n):
    """the level shapes of mg_build_levels on one rank: every axis whose cell count is even and >= 8 is halved, until none is"""
    levels = [tuple(n)]
    while True:
        r = [2 if m % 2 == 0 and m >= 8 else 1 for m in levels[-1]]
        if max(r) == 1:
            return levels
        levels.append(tuple(m // q for m, q in zip(levels[-1], r)))


def _chunks(n, size):
    """lengths of the pieces of n cells cut into pieces of size"""
    return [min(size, n - a) for a in range(0, n, size)]


def mg_trips(items):
    """grid-stride trips (items per thread of the whole grid) of a 256-thread kernel whose grid is capped at MG_BLOCKS (nblk in fl_mg.hip)"""
    return items / (256 * max(1, min(-(-items // 256), MG_BLOCKS)))


def mg_plans(n):
    """per level of the hierarchy on an n block, what the cycle runs there (host arithmetic of vcycle and fl_solve_cg_mg):
      n, cells, ratio (to the next level; None on the coarsest), cg.regime and cg.nw of the level's own plan_cg_A, rr.fused (mg_restrict_fused),
      smoother: "fused" (k_cheb2, the three steps from zero in one sweep) or "single" (k_cheb_st);
    on a level with a coarser one
      rr: "fused" (k_bcgs_st MODE 11 on the level's plan) or "fallback" (the residual, then k_mg_restrict: restrict_trips grid-stride trips),
      prolong: "cc" (k_mg_prolong_lin_cc, every axis halved: prolong.xblocks of 62 coarse columns, prolong.zchunks of 4 coarse planes) or "tile"
      (k_mg_prolong_lin_tile<false>: x tiles of 128 fine columns, z chunks of 8 fine planes);
    on the coarsest level
      coarse: "coarse_cg" (k_mg_coarse_cg) or "pcg" (the public Jacobi-PCG);
    on level 0
      pw_trips: the grid-stride trips of k_mg_pwd and k_mg_dots (a thread per cell pair)"""
    levels = mg_levels(n)
    out = []
    for l, m in enumerate(levels):
        p = launch_plans(m)
        cells = m[0] * m[1] * m[2]
        lv = {"n": m, "cells": cells, "ratio": None, "cg.regime": p["cg.regime"], "cg.nw": p["cg.nw"], "rr.fused": mg_restrict_fused(m),
              "smoother": "fused" if cells >= CHEB2_MIN_CELLS and min(m) >= 2 else "single"}
        if l == 0:
            lv["pw_trips"] = mg_trips((m[0] + 1) // 2 * m[1] * m[2])
        if l + 1 == len(levels):
            lv["coarse"] = "coarse_cg" if cells <= MG_COARSE_MAX else "pcg"
        else:
            c = levels[l + 1]
            lv["ratio"] = tuple(a // b for a, b in zip(m, c))
            full = lv["ratio"] == (2, 2, 2)
            lv["rr"] = "fused" if full and lv["rr.fused"] else "fallback"
            if lv["rr"] == "fallback":
                lv["restrict_trips"] = mg_trips(c[0] * c[1] * c[2])
            if full:
                lv.update({"prolong": "cc", "prolong.xblocks": _chunks(c[0], 62), "prolong.zchunks": _chunks(c[2], 4)})
            else:
                lv.update({"prolong": "tile", "prolong.xblocks": _chunks(m[0], 128), "prolong.zchunks": _chunks(m[2], 8)})
        out.append(lv)
    return out


def mg_summary(n):
    """{mg.<field>: value} of the hierarchy on an n block: its depth, the levels that take the one-pass residual + restriction, the coarse solve"""
    lv = mg_plans(n)
    return {"mg.levels": len(lv), "mg.rr_fused": tuple(l for l, v in enumerate(lv) if v.get("rr") == "fused"), "mg.coarse": lv[-1]["coarse"]}


class Regime:
    def __init__(self, name, n, bcs, expect, reaches, mg=None):
        # mg: the multigrid regimes only -- per level of mg_plans(n), the fields that level must have (one dict per level, the coarsest included)
        self.name, self.n, self.bcs, self.expect, self.reaches, self.mg = name, tuple(n), bcs, expect, reaches, mg

    def __repr__(self):
        return f"{self.name} {self.n[0]}x{self.n[1]}x{self.n[2]}"


REGIMES = [
    Regime("cg_standard_ragged", (300, 680, 21), [CAVITY, XPER],
           {"cg.regime": "standard", "cg.ry": 2, "cg.nw": 8, "cg.tiles_x": 3, "cg.tiles_y": 43, "cg.nchunk": 2, "cg.zc": 11, "cg.nblocks": 258,
            "cheb2.nw": 8, "cheb2.tiles": 129, "cheb2.nchunk": 1, "cheb2.clamp": 1,
            "six.nxcd": 8, "six.nbx": 1026, "six.items": 5355,
            "schur.per_xcd": 128, "schur.fixed_seg": 0},
           "tiles16 = 129 in 8-wave tiles (x: 2 full tiles + 44 columns, y: 42.5 tiles); z chunks of 11 + 10; cheb2 clamp; "
           "project-six 1.3 trips; schur 128 blocks per XCD, general segments"),
    Regime("cg_mid_ragged", (300, 200, 280), [CHANNEL, XPER],
           {"cg.regime": "mid", "cg.ry": 2, "cg.nw": 8, "cg.tiles_x": 3, "cg.tiles_y": 13, "cg.nchunk": 6, "cg.zc": 47, "cg.nblocks": 234,
            "cheb2.nw": 8, "cheb2.tiles": 39, "cheb2.nchunk": 6, "cheb2.zc": 47, "cheb2.nblocks": 234, "cheb2.clamp": 1,
            "six.nxcd": 8, "six.nbx": 1026, "six.items": 21000},
           "2^24 cells and more with 39 tiles of 128 x 16: 6 z chunks of 47, the last 45; cheb2 clamp with 6 chunks; project-six 5.1 trips"),
    Regime("schur_fixed_seg", (200, 37, 40), [CAVITY],
           {"cg.regime": "small_ry1", "schur.per_xcd": 128, "schur.nseg": 4, "schur.fixed_seg": 1, "schur.band": 5},
           "schur: 128 blocks per XCD, every wave keeps one x segment (the last one 8 cells wide), y bands of 5 with a last band of 2"),
    Regime("schur_general", (300, 37, 40), [XPER],
           {"cg.regime": "small", "schur.per_xcd": 128, "schur.nseg": 5, "schur.fixed_seg": 0, "schur.band": 5},
           "schur: 128 blocks per XCD, a wave's x segment changes from row to row"),
    # the t2 tiling of the momentum kernels (k_mom3, k_mom2, k_mom_pw3): 128 x 8 tiles, z chunks, XCD-contiguous block order when the blocks
    # are a multiple of 8.  tests/test_gpu_momentum_regimes.py runs them on these grids, stretched in all three axes.
    Regime("mom_long_chunks", (3, 505, 879), [CHANNEL],
           {"mom.t2x": 1, "mom.t2chunk": 16, "mom.t2zc": 55, "mom.t2blocks": 1024},
           "t2: the tile bound like 384^3 -- 64 tiles, 16 z chunks of 55 planes with a last one of 54, 1024 blocks so the XCD remap is on; "
           "one x tile holds both x ends; a last y tile of 1 row; the periodic z seam crosses the chunks"),
    Regime("mom_three_tiles", (257, 17, 71), [CAVITY, XPER],
           {"mom.t2x": 3, "mom.t2chunk": 8, "mom.t2zc": 9, "mom.t2blocks": 72},
           "t2: x tiles of 128 / 128 / 1 column and y tiles of 8 / 8 / 1 row, so one tile touches no block end; 8 z chunks of 9, the last 8; "
           "72 blocks, remapped; the periodic x seam joins the 1-column tile to tile 0"),
    Regime("mom_pairs_one_plane", (256, 41, 100), [CHANNEL],
           {"mom.t2x": 2, "mom.t2chunk": 12, "mom.t2zc": 9, "mom.t2blocks": 144},
           "t2: nx a multiple of 128 -- a full last x tile and 16-byte pair stores (flags & 2); 12 z chunks of 9 with a last chunk of one plane; "
           "144 blocks, remapped; a last y tile of 1 row"),
    Regime("mom_unmapped", (130, 37, 43), [CAVITY],
           {"mom.t2x": 2, "mom.t2chunk": 5, "mom.t2zc": 9, "mom.t2blocks": 50},
           "t2: 50 blocks, so the block order is not remapped; 5 z chunks of 9, the last 7; x tiles of 128 / 2 columns, a last y tile of 5 rows"),
    Regime("mom_stored_one_plane", (300, 8, 100), [SLAB],
           {"mom.t2x": 3, "mom.t2chunk": 12, "mom.t2zc": 9, "mom.t2blocks": 36},
           "t2 with ny = 8: one tile holds both y ends, so k_mom2 runs also for a state with v0; 12 z chunks of 9 with a last chunk of one plane; "
           "36 blocks, not remapped; x tiles of 128 / 128 / 44"),
    # the multigrid cycle (mg_plans): the one-pass residual + restriction, the prolongations, the grid-stride kernels and both coarse solves in
    # the plans of 256^3 - 512^3.  tests/test_gpu_mg_regimes.py runs MG-PCG on these grids, uniform and stretched in all three axes.
    Regime("mg_standard", (304, 680, 28), [CAVITY, XPER],
           {"cg.regime": "standard", "cg.nw": 8, "cg.tiles_x": 3, "cg.tiles_y": 43, "cg.nchunk": 2, "cg.zc": 14, "cg.nblocks": 258},
           "L0 in the standard plan: 129 tiles of 8 waves (x tiles of 128 / 128 / 48, a half y tile), 2 z chunks of 14, the one-pass kernel with 8 "
           "waves; lin_cc onto 152 x 340 x 14 with x blocks of 62 / 62 / 28 and z chunks of 4 / 4 / 4 / 2; L1's z chunks are odd: the fallback; "
           "then (2,2,1) and (2,1,1) and a coarsest level of 11305 cells (the public PCG)",
           mg=[{"n": (304, 680, 28), "ratio": (2, 2, 2), "cg.regime": "standard", "cg.nw": 8, "rr.fused": 1, "rr": "fused", "smoother": "fused", "prolong": "cc",
                "prolong.xblocks": [62, 62, 28], "prolong.zchunks": [4, 4, 4, 2]},
               {"n": (152, 340, 14), "ratio": (2, 2, 2), "cg.nw": 4, "rr.fused": 0, "rr": "fallback", "smoother": "fused", "prolong": "cc",
                "prolong.xblocks": [62, 14], "prolong.zchunks": [4, 3]},
               {"n": (76, 170, 7), "ratio": (2, 2, 1), "rr": "fallback", "smoother": "fused", "prolong": "tile"},
               {"n": (38, 85, 7), "ratio": (2, 1, 1), "rr": "fallback", "smoother": "single", "prolong": "tile"},
               {"n": (19, 85, 7), "cells": 11305, "coarse": "pcg"}]),
    Regime("mg_mid", (288, 392, 160), [CHANNEL],
           {"cg.regime": "mid", "cg.nw": 8, "cg.tiles_x": 3, "cg.tiles_y": 25, "cg.nchunk": 3, "cg.zc": 54},
           "L0 in the mid plan: 8 waves, z chunks of 54 / 54 / 52; the one-pass kernel on L0 (8 waves), L1 and L2 (4 waves); lin_cc with x blocks "
           "of 62 / 62 / 20; then (2,1,2) twice and a coarsest level of 2205 cells (k_mg_coarse_cg)",
           mg=[{"n": (288, 392, 160), "ratio": (2, 2, 2), "cg.regime": "mid", "cg.nw": 8, "rr.fused": 1, "rr": "fused", "smoother": "fused", "prolong": "cc",
                "prolong.xblocks": [62, 62, 20]},
               {"n": (144, 196, 80), "ratio": (2, 2, 2), "cg.nw": 4, "rr": "fused", "prolong": "cc"},
               {"n": (72, 98, 40), "ratio": (2, 2, 2), "cg.nw": 4, "rr": "fused", "prolong": "cc"},
               {"n": (36, 49, 20), "ratio": (2, 1, 2), "rr": "fallback", "prolong": "tile", "prolong.zchunks": [8, 8, 4]},
               {"n": (18, 49, 10), "ratio": (2, 1, 2), "rr": "fallback", "prolong": "tile"},
               {"n": (9, 49, 5), "cells": 2205, "coarse": "coarse_cg"}]),
    Regime("mg_semi", (304, 208, 273), [XPER],
           {"cg.regime": "mid", "cg.nw": 8, "cg.tiles_x": 3, "cg.tiles_y": 13, "cg.nchunk": 6, "cg.zc": 46},
           "(2,2,1) at 17 M cells: the fallback residual on the mid 8-wave plan, then k_mg_restrict over 4096 blocks (4.1 trips); "
           "lin_tile<false> with x tiles of 128 / 128 / 48 and z chunks of 8, the last one a single plane; z is never coarsened: a coarsest level of "
           "67431 cells (the public PCG, which ends on its 200 iterations there, short of rtol 1e-2)",
           mg=[{"n": (304, 208, 273), "ratio": (2, 2, 1), "cg.regime": "mid", "cg.nw": 8, "rr.fused": 0, "rr": "fallback", "smoother": "fused", "prolong": "tile",
                "prolong.xblocks": [128, 128, 48], "prolong.zchunks": [8] * 34 + [1]},
               {"n": (152, 104, 273), "ratio": (2, 2, 1), "prolong": "tile", "prolong.xblocks": [128, 24]},
               {"n": (76, 52, 273), "ratio": (2, 2, 1), "prolong": "tile"},
               {"n": (38, 26, 273), "ratio": (2, 2, 1), "prolong": "tile"},
               {"n": (19, 13, 273), "cells": 67431, "coarse": "pcg"}]),
    Regime("production_256", (256, 256, 256), [CAVITY],
           {"cg.regime": "mid", "cg.nw": 8, "cg.nchunk": 8, "cg.zc": 32},
           "exactly what a 256^3 solve runs: the one-pass kernel on L0 (8 waves), L1 and L2 (4 waves), the fallback from 32^3 on; lin_cc onto 128^3 "
           "with x blocks of 62 / 62 / 4; 7 levels down to 4^3 (k_mg_coarse_cg)",
           mg=[{"n": (256, 256, 256), "ratio": (2, 2, 2), "cg.nw": 8, "rr.fused": 1, "rr": "fused", "prolong": "cc", "prolong.xblocks": [62, 62, 4]},
               {"n": (128, 128, 128), "cg.nw": 4, "rr": "fused"},
               {"n": (64, 64, 64), "cg.nw": 4, "rr": "fused"},
               {"n": (32, 32, 32), "cg.regime": "small_ry1", "rr": "fallback", "smoother": "fused"},
               {"n": (16, 16, 16), "rr": "fallback", "smoother": "single"},
               {"n": (8, 8, 8), "rr": "fallback"},
               {"n": (4, 4, 4), "cells": 64, "coarse": "coarse_cg"}]),
]
BY_NAME = {r.name: r for r in REGIMES}

# the shapes the product runs (512^3 bench, config 5's 512 x 512 x 256 blocks, the multigrid fine levels of 384^3 and 256^3): which plans they take
PRODUCTION = {
    (512, 512, 512): {"cg.regime": "standard", "cg.nblocks": 256, "cg.nchunk": 2, "cheb2.nchunk": 2, "cheb2.clamp": 0, "six.nbx": 1024,
                      "six.items": 131072, "schur.per_xcd": 128, "schur.fixed_seg": 1, "mom.t2chunk": 4,
                      "mom.t2x": 4, "mom.t2zc": 128, "mom.t2blocks": 1024},
    (512, 512, 256): {"cg.regime": "standard", "cg.nblocks": 256, "cg.nchunk": 2, "cheb2.nchunk": 2, "cheb2.clamp": 0, "six.nbx": 1024,
                      "six.items": 65536, "schur.per_xcd": 128, "schur.fixed_seg": 1, "mom.t2chunk": 4,
                      "mom.t2x": 4, "mom.t2zc": 64, "mom.t2blocks": 1024},
    (384, 384, 384): {"cg.regime": "mid", "cg.nblocks": 216, "cg.nchunk": 3, "cheb2.nchunk": 3, "cheb2.clamp": 1, "six.nbx": 1026,
                      "six.items": 55296, "schur.per_xcd": 128, "schur.fixed_seg": 0, "mom.t2chunk": 7,
                      "mom.t2x": 3, "mom.t2zc": 55, "mom.t2blocks": 1008},
    (256, 256, 256): {"cg.regime": "mid", "cg.nblocks": 256, "cg.nchunk": 8, "cheb2.nchunk": 8, "cheb2.clamp": 0, "six.nbx": 1024,
                      "six.items": 16384, "schur.per_xcd": 128, "schur.fixed_seg": 1, "mom.t2chunk": 16,
                      "mom.t2x": 2, "mom.t2zc": 16, "mom.t2blocks": 1024},
}
# and the multigrid hierarchy a single-rank solve builds on them (mg_summary): its depth, the levels that take the one-pass residual + restriction,
# the coarse solve
PRODUCTION_MG = {
    (512, 512, 512): {"mg.levels": 8, "mg.rr_fused": (0, 1, 2, 3), "mg.coarse": "coarse_cg"},
    (512, 512, 256): {"mg.levels": 8, "mg.rr_fused": (0, 1, 2), "mg.coarse": "coarse_cg"},
    (384, 384, 384): {"mg.levels": 7, "mg.rr_fused": (0, 1), "mg.coarse": "coarse_cg"},
    (256, 256, 256): {"mg.levels": 7, "mg.rr_fused": (0, 1, 2), "mg.coarse": "coarse_cg"},
}


# ---- several ranks: rank grids whose BLOCKS take the plans of 256^3 - 512^3.  What a rank of a several-rank solve runs differently from one rank
# -- q stored on the block's six boundary layers only (PlanA::qb), the neighbour's ghost of r formed from them, the two-deep exchange under
# k_cheb2, k_project_six<false> on the padded p, k_schur_var_ring -- meets the ragged tile, chunk and band edges only on such blocks.
class RankRegime:
    def __init__(self, name, n, ranks, own, bcs, blocks, expect, reaches):
        # own: ownership ranges per axis, None = the DMStag default split (mp_common.decomp_of); blocks: the block of every rank, in rank order
        # (x fastest); expect: the plan fields every block must get, or one dict per rank
        self.name, self.n, self.ranks, self.own, self.bcs, self.blocks, self.reaches = name, tuple(n), tuple(ranks), own, bcs, blocks, reaches
        self.expect = expect if isinstance(expect, list) else [expect] * len(blocks)
        assert len(self.blocks) == len(self.expect) == ranks[0] * ranks[1] * ranks[2]

    def __repr__(self):
        return f"{self.name} {self.n[0]}x{self.n[1]}x{self.n[2]} on {self.ranks[0]}x{self.ranks[1]}x{self.ranks[2]} ranks"

    def decomp(self, rank):
        """the fl_decomp of a rank: the default split, or the ownership ranges"""
        from fluca_amd import capi
        from tests import mp_common as mpc
        return mpc.decomp_of(capi, self.n, self.ranks, rank, self.own)

    def periodic(self, bc):
        return [bc[2 * a] == PER for a in range(3)]


_RSTD = {"cg.regime": "standard", "cg.ry": 2, "cg.nw": 8, "cg.tiles_x": 3, "cg.tiles_y": 43, "cg.nchunk": 2, "cg.zc": 11, "cg.nblocks": 258,
         "cheb2.nw": 8, "cheb2.tiles": 129, "cheb2.nchunk": 1, "cheb2.clamp": 1, "six.nbx": 1026, "six.items": 5355}
_RMID = {"cg.regime": "mid", "cg.ry": 2, "cg.nw": 8, "cg.tiles_x": 3, "cg.tiles_y": 13, "cg.nchunk": 6, "cg.zc": 47, "cg.nblocks": 234,
         "cheb2.nw": 8, "cheb2.tiles": 39, "cheb2.nchunk": 6, "cheb2.zc": 47, "cheb2.clamp": 1, "six.nbx": 1026}
_RSF = {"cg.regime": "small_ry1", "schur.per_xcd": 128, "schur.nseg": 4, "schur.fixed_seg": 1, "schur.band": 5}
_RSG = {"cg.regime": "small", "schur.per_xcd": 128, "schur.nseg": 5, "schur.fixed_seg": 0, "schur.band": 5}

RANK_REGIMES = [
    RankRegime("ranks_std_z", (300, 680, 42), (1, 1, 2), None, [CAVITY, CHANNEL], [(300, 680, 21)] * 2, _RSTD,
               "the 2-GPU layout of the bench: the exchanged face is a whole 300 x 680 plane; the stored q planes are plane 0 (first of chunk 0) and "
               "plane 20 (last of the short chunk of 10); CHANNEL: z periodic across the two ranks (the same peer on both sides)"),
    RankRegime("ranks_std_z3", (300, 680, 63), (1, 1, 3), None, [CAVITY, CHANNEL], [(300, 680, 21)] * 3, _RSTD,
               "an interior block in the standard plan: the middle rank has a different peer below and above, its stored q planes 0 and 20 go to two "
               "ranks, it has no wall row in z; CHANNEL: z periodic over three ranks, the seam joins rank 2 to rank 0"),
    RankRegime("ranks_std_xy", (601, 1359, 21), (2, 2, 1), None, [XPER, CAVITY], [(301, 680, 21), (300, 680, 21), (301, 679, 21), (300, 679, 21)], _RSTD,
               "2 x 2 ranks: the edge cells of the deep exchange travel in two hops; blocks with odd nx (301: the last cell alone in its lane's pair) "
               "and odd ny (679: the last row alone in its wave's pair); XPER: x periodic across ranks, z wraps inside the block"),
    RankRegime("ranks_mid_y", (300, 401, 281), (1, 2, 1), None, [CHANNEL], [(300, 201, 281), (300, 200, 281)], _RMID,
               "a y face of 300 x 281 cells across the 6 z chunks of the mid plan (5 x 47 + 46); the last row of the low block (201 rows) sits alone in "
               "its wave's pair of rows in a partial y tile; z periodic inside the block across the chunks"),
    RankRegime("ranks_mid_x", (601, 200, 280), (2, 1, 1), None, [XPER], [(301, 200, 280), (300, 200, 280)], _RMID,
               "an x face of 200 x 280 cells across the 6 z chunks (5 x 47 + 45), x periodic across the two ranks; the last cell of the 301 block "
               "alone in its lane's pair, in the partial x tile"),
    # k_schur_var_ring at 128 blocks per XCD: the blocks are those of the schur_fixed_seg and schur_general regimes, split along each axis in turn
    # (the x split of that block, 400 x 37 x 40, is no use: the momentum kernels form diag(A) of the x component by another code path in the first, the
    # inner and the last 128-column tile of a block, 2 ulp apart in a quarter of the cells; in 256 of the 400 columns a rank's tile is of another kind than
    # the one-rank tile, and tests/test_gpu_schur_var_multirank.py::_same_bits then finds 34 % of the cells next to such an entry, above its cap of a
    # quarter (measured).  Blocks of 456 columns -- eight segments, the last one again 8 cells wide -- leave 256 such columns of 912: 15 %)
    RankRegime("ranks_schur_fixed_x", (912, 37, 40), (2, 1, 1), ([456, 456], [37], [40]), [CAVITY], [(456, 37, 40)] * 2,
               {"cg.regime": "small", "schur.per_xcd": 128, "schur.nseg": 8, "schur.fixed_seg": 1, "schur.band": 5},
               "a wave keeps its x segment (eight of them, the last one 8 cells wide): the x split puts the ring into the rows a wave loads once"),
    RankRegime("ranks_schur_fixed_y", (200, 74, 40), (1, 2, 1), ([200], [37, 37], [40]), [CAVITY], [(200, 37, 40)] * 2, _RSF,
               "the ring rows below / above the y bands of 5 with a last band of 2"),
    RankRegime("ranks_schur_fixed_z", (200, 37, 80), (1, 1, 2), ([200], [37], [40, 40]), [CAVITY], [(200, 37, 40)] * 2, _RSF,
               "the ring planes; a symmetry plane and a wall at the two outer z ends"),
    RankRegime("ranks_schur_general_x", (600, 37, 40), (2, 1, 1), ([300, 300], [37], [40]), [XPER], [(300, 37, 40)] * 2, _RSG,
               "a wave's x segment changes from row to row; x periodic across the two ranks (the same peer on both sides)"),
    RankRegime("ranks_schur_general_z", (300, 37, 80), (1, 1, 2), ([300], [37], [40, 40]), [XPER], [(300, 37, 40)] * 2, _RSG,
               "z periodic across the two ranks, x wraps inside the block"),
]
RANK_BY_NAME = {r.name: r for r in RANK_REGIMES}

# the blocks of the several-rank tests on toy grids (tests/test_gpu_multirank.py, tests/test_gpu_config5.py, tests/test_gpu_schur_var_multirank.py): none
# takes an 8-wave plan
TOY_RANK_BLOCKS = [(24, 20, 8), (12, 20, 16), (24, 10, 16), (70, 18, 12), (68, 20, 12), (70, 6, 10), (20, 18, 12), (16, 16, 16), (24, 16, 16),
                   (12, 20, 8), (16, 16, 8), (8, 16, 8),                                                             # test_gpu_multirank
                   (32, 24, 16), (21, 19, 15), (20, 18, 14), (24, 20, 16), (20, 16, 12), (64, 32, 16), (64, 32, 15),   # test_gpu_config5
                   (5, 9, 8), (8, 9, 8), (9, 6, 4), (9, 7, 7), (5, 6, 3), (7, 5, 7), (7, 6, 7), (12, 16, 12),          # test_gpu_schur_var_multirank
                   (4, 9, 8), (9, 6, 7), (9, 3, 7), (10, 9, 4), (10, 9, 6), (10, 9, 5),                                # ... its three-rank cases
                   (10, 12, 8), (12, 8, 9), (12, 7, 9), (7, 10, 8), (16, 12, 6), (16, 12, 4), (16, 12, 5), (9, 8, 8),
                   (32, 32, 32), (32, 32, 31)]                                                                         # test_gpu_interior_ranks
