"""The regime table of tests/launch_regimes.py against the plans the library computes (fldbg_launch_plans: host arithmetic, no GPU).

If a threshold of a plan moves, these tests name the regime whose grid no longer reaches its branch: the -m gpu module
tests/test_gpu_launch_regimes.py then checks another plan than the one it was written for, and the table must be re-aimed."""
import pytest

from tests.launch_regimes import BY_NAME, FIELDS, PRODUCTION, REGIMES, launch_plans, six_trips


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
