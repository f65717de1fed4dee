"""-m gpu: the x-flush of k_cg_Bq at the deep direction rings (cg_xdepth = 8 and 16).  The flush loads x and the older directions inside
the step that updates them, the sixteen-deep ring in two groups; whatever the depth and whatever iteration the solve stops on, x and the
residual norm must be bit for bit those of one update per iteration (cg_xbatch = 0)."""
import numpy as np
import pytest
import torch

from fluca_amd import capi
from tests.gpu_common import CAVITY, PER, dev, host, make_pair, mean_free_rhs
from tests.launch_regimes import BY_NAME, launch_plans

pytestmark = pytest.mark.gpu

K16 = 16
GRIDS = [
    ((17, 9, 11), CAVITY),
    ((12, 10, 9), [PER] * 6),
    ((130, 37, 20), CAVITY),   # > 1 tile in x and y, 2 z-chunks, ragged edges
]
STD = BY_NAME["cg_standard_ragged"]   # (300, 680, 21): 3 x 43 tiles of 128 x 16 (8 waves), z chunks of 11 + 10, ragged in x, y and z


def _knob(name, value):
    capi.check(capi.lib.fl_tuning_set(name, value), "fl_tuning_set")


def _knob_get(name):
    import ctypes as C
    v = C.c_int(0)
    capi.check(capi.lib.fl_tuning_get(name, C.byref(v)), "fl_tuning_get")
    return v.value


@pytest.fixture
def restore_knobs():
    keep = {k: _knob_get(k) for k in (b"cg_xdepth", b"cg_xbatch")}
    yield
    for k, v in keep.items():
        _knob(k, v)


def _one_per_iteration(P, bd, **kw):
    _knob(b"cg_xbatch", 0)
    try:
        return P.solve(bd, **kw)
    finally:
        _knob(b"cg_xbatch", 1)


@pytest.mark.parametrize("n,bc", GRIDS)
def test_depth16_stopped_after_any_iteration(n, bc, restore_knobs):
    P, g = make_pair(n, bc, kappa=1e-3)
    _, b = mean_free_rhs(g.assemble_S(), g.ncell)
    bd = dev(b)
    _knob(b"cg_xdepth", K16)
    for maxit in range(1, 2 * K16 + 4):
        kw = dict(rtol=0.0, atol=0.0, maxit=maxit, check_every=3)
        x1, i1 = _one_per_iteration(P, bd, **kw)
        x0, i0 = P.solve(bd, **kw)
        assert i0["iters"] == maxit and i0["reason"] == -3
        assert torch.equal(x0, x1) and i0["rnorm"] == i1["rnorm"], maxit
    P.close()


@pytest.mark.parametrize("n,bc", GRIDS)
def test_depth16_converged_on_every_residue(n, bc, restore_knobs):
    P, g = make_pair(n, bc, kappa=1e-3)
    S = g.assemble_S()
    _, b = mean_free_rhs(S, g.ncell)
    bd = dev(b)
    _, info = P.solve(bd, rtol=0.0, atol=0.0, maxit=40, history=True)
    h = info["history"]
    rel = h / h[0]
    _knob(b"cg_xdepth", K16)
    for stop in range(6, 6 + K16):
        rtol = rel[stop] * (1 + 1e-12)
        want = int(np.argmax(rel <= rtol))          # the first iteration whose norm passes the test
        x0, i0 = P.solve(bd, rtol=rtol, atol=0.0, maxit=100)
        assert i0["reason"] == 2 and i0["iters"] == want, stop
        x1, i1 = _one_per_iteration(P, bd, rtol=rtol, atol=0.0, maxit=100)
        assert torch.equal(x0, x1) and i0["rnorm"] == i1["rnorm"], stop
        xo, io = S.solve(b, rtol=rtol)
        assert io["reason"] == 2 and abs(io["iters"] - i0["iters"]) <= 1
        if io["iters"] == i0["iters"]:
            assert np.abs(host(x0) - xo).max() <= 1e-9 * np.abs(xo).max(), stop
    P.close()


def test_eight_wave_instances_flush_bit_for_bit(restore_knobs):
    """Small grids never reach the 8-wave kernels.  K - 1 iterations never flush (x_valid = 0), K flush without reading x, the others leave
    owed updates to k_cg_finish."""
    from fluca_amd.poisson import Poisson
    from tests.gpu_common import CAVITY_BOX
    plan = launch_plans(STD.n)
    assert (plan["cg.nw"], plan["cg.ry"], plan["cg.tiles_x"], plan["cg.tiles_y"], plan["cg.nchunk"], plan["cg.zc"]) == (8, 2, 3, 43, 2, 11)
    P = Poisson.uniform(STD.n, CAVITY_BOX, CAVITY, 1e-3)
    gen = torch.Generator(device="cuda").manual_seed(20260313)
    bd = torch.rand(P.ncell, generator=gen, device="cuda", dtype=torch.float64) * 2 - 1
    bd -= bd.mean()
    ref = {}
    for K in (8, K16):
        _knob(b"cg_xdepth", K)
        for maxit in (K - 1, K, K + 1, 2 * K, 2 * K + 3):
            kw = dict(rtol=0.0, atol=0.0, maxit=maxit)
            if maxit not in ref:
                ref[maxit] = _one_per_iteration(P, bd, **kw)
            x1, i1 = ref[maxit]
            x0, i0 = P.solve(bd, **kw)
            assert i0["iters"] == maxit and i0["reason"] == -3
            assert torch.equal(x0, x1) and i0["rnorm"] == i1["rnorm"], (K, maxit)
    P.close()


def test_second_solve_on_one_handle_matches_a_fresh_handle(restore_knobs):
    """The ring slots keep the finite leftovers of the solve before: a solve that follows one which stopped with updates owed must not see them."""
    n, bc = GRIDS[2]
    _knob(b"cg_xdepth", K16)
    P, g = make_pair(n, bc, kappa=1e-3)
    _, b = mean_free_rhs(g.assemble_S(), g.ncell)
    bd = dev(b)
    kw = dict(rtol=0.0, atol=0.0, maxit=2 * K16 + 5)
    _, i0 = P.solve(bd, rtol=0.0, atol=0.0, maxit=K16 + 3)   # stops with three updates owed, every slot of the ring written
    assert i0["iters"] == K16 + 3
    x2, i2 = P.solve(bd, **kw)
    P.close()
    Q, _ = make_pair(n, bc, kappa=1e-3)
    xf, jf = Q.solve(bd, **kw)
    Q.close()
    assert i2["iters"] == jf["iters"] == 2 * K16 + 5
    assert torch.equal(x2, xf) and i2["rnorm"] == jf["rnorm"]
