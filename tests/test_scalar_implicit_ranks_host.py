"""The implicit scalar diffusion on several ranks, without a GPU: include/fluca_hip_implicit_ranks.h against the ctypes table and the exports, the stream-order
rows of its three functions, the host mirror's new call, and the numpy side of the GPU tests -- the cases scatter and gather, and the wire counted from
geometry (tests/scalar_implicit_ranks.py) agrees with half the bytes of the two-plane exchange of tests/scalar_ranks.py."""
import os
import re

import numpy as np
import pytest

from tests import scalar_implicit_ranks as irk
from tests import scalar_ranks as rk
from tests import stream_order as so
from tests.test_stream_order import problems

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("fl_scalar_diffusion_apply_ranks", "fl_scalar_diffusion_solve_ranks", "fl_scalar_step_imex_ranks")


@pytest.fixture(scope="module")
def capi():
    from fluca_amd import capi
    return capi


def ranks_header():
    return open(os.path.join(ROOT, "include", "fluca_hip_implicit_ranks.h")).read()


def test_header_table_and_exports_name_the_same_functions(capi):
    decl = so.declarations(ranks_header())
    assert sorted(decl) == sorted(capi.PROTOTYPES_IMPLICIT_RANKS) == sorted(NAMES)
    for name, (params, comment) in decl.items():
        assert hasattr(capi.lib, name), name
        assert len(params) == len(capi.PROTOTYPES_IMPLICIT_RANKS[name][1]), name
        assert comment.strip(), f"{name} has no comment"
        # the collective call takes what the one-rank call takes
        plain = so.declarations(open(os.path.join(ROOT, "include", "fluca_hip_implicit.h")).read())[name[:-len("_ranks")]][0]
        assert list(params) == list(plain), name
    for other in (capi.PROTOTYPES, capi.PROTOTYPES_IMPLICIT, capi.PROTOTYPES_IBM_SCALAR):
        assert not set(capi.PROTOTYPES_IMPLICIT_RANKS) & set(other)
    assert '#include "fluca_hip_implicit.h"' in ranks_header()
    for hdr in ("fluca_hip.h", "fluca_hip_implicit.h"):
        assert not re.search(r"int fl_\w+_ranks\(fl_scalar", open(os.path.join(ROOT, "include", hdr)).read()), hdr
    # not part of the public header, and exported for tools/scalar_implicit_bench.py --ring
    assert hasattr(capi.lib, "fldbg_scalar_cheb_ring_one") and "fldbg_" not in ranks_header()


TABLE = {
    "fl_scalar_diffusion_apply_ranks": (so.ASYNC, dict(phi_dev=so.C, out_dev=so.C)),
    "fl_scalar_diffusion_solve_ranks": (so.ASYNC, dict(b_dev=so.C, x_dev=so.C, info=so.C)),
    "fl_scalar_step_imex_ranks": (so.ASYNC, dict(source_dev=so.C, phi_dev=so.C, info=so.C)),
}


def test_stream_order_rows_of_the_new_functions():
    header = ranks_header()
    assert problems(TABLE, header) == []
    decl = so.declarations(header)
    for name in NAMES:
        assert "CONSUMED" in decl[name][1] and re.search(r"Wire: ", decl[name][1]), name
    assert re.search(r"ordered on the handle's stream", header) and "all-reduce" in header
    short = dict(TABLE)
    del short["fl_scalar_step_imex_ranks"]
    assert len(problems(short, header)) == 1


def test_null_handles(capi):
    import ctypes as C
    x = C.c_void_p(4096)                       # never dereferenced: the handle is checked first
    assert capi.lib.fl_scalar_diffusion_apply_ranks(None, 1.0, x, x) == -85
    assert capi.lib.fl_scalar_diffusion_solve_ranks(None, 1.0, 1e-6, 10, x, x, None) == -85
    assert capi.lib.fl_scalar_step_imex_ranks(None, 0.1, 3, 1.0, 1e-6, 10, None, x, None) == -85


def test_the_host_mirror_declares_and_binds_the_new_call():
    hdr = open(os.path.join(ROOT, "include", "fluca_host.h")).read()
    assert re.search(r"FlErrorCode NSSetScalarImplicitRanks\(NS ns, int id, double theta, double rtol\);", hdr)
    assert re.search(r"FlErrorCode NSSetScalarImplicit\(NS ns, int id, double theta, double rtol\);", hdr)
    assert "-ns_scalar_implicit_ranks" in hdr and '#include "fluca_hip_implicit_ranks.h"' in hdr
    from fluca_amd import hostapi
    H = hostapi.lib
    assert H.NSSetScalarImplicitRanks.argtypes == H.NSSetScalarImplicit.argtypes
    assert H.NSSetScalarImplicitRanks(None, 0, 1.0, 1e-6) != 0          # no NS: an error, not a crash
    src = open(os.path.join(ROOT, "fluca_amd", "host", "fluca_host.c")).read()
    assert "fl_scalar_step_imex_ranks(sc->h" in src and "fl_scalar_step_imex(sc->h" in src


def test_the_build_knows_the_header():
    from fluca_amd import build
    assert any(h.endswith("fluca_hip_implicit_ranks.h") for h in build.HEADERS)
    text = open(os.path.join(ROOT, "fluca_amd", "build.py")).read()
    assert text.count('"fluca_hip_implicit_ranks.h"') == 4                      # libflucahip.so, the host mirror, the CGNS dump, the examples


CASES = irk.cases()


def test_the_cases_are_the_ones_listed():
    ids = [rk.case_id(c) for c in CASES]
    assert len(ids) == 24
    assert sum(i.startswith("4x4x4-") for i in ids) == 3 and sum(i.startswith("130x6x7-") for i in ids) == 3
    assert sum(i.startswith("7x5x6-2x1x1-") for i in ids) == 8 and sum(i.startswith("7x6x5-2x2x2-") for i in ids) == 4
    assert sum(i.startswith("6x5x4-3x1x1-") for i in ids) == 2 and sum(i.startswith("4x5x6-1x1x3-") for i in ids) == 2
    last, cap = CASES[-2], CASES[-1]
    assert last.n == (65, 64, 80) and tuple(last.lo_len(0)[1]) == tuple(last.lo_len(1)[1]) == irk.PLAN_BLOCK
    assert cap.n == (65, 64, 130) and tuple(cap.lo_len(0)[1]) == tuple(cap.lo_len(1)[1]) == irk.CAP_BLOCK
    assert all(min(c.lo_len(r)[1]) >= 2 for c in CASES for r in range(c.size))       # (fl_scalar_create_ranks refuses a one-cell block along a split axis)
    assert all(c.size <= 8 for c in CASES)


@pytest.mark.parametrize("case", CASES, ids=rk.case_id)
def test_scatter_then_gather_is_the_identity(case):
    rng = np.random.default_rng(5)
    a = rng.uniform(-1, 1, case.shp)
    blocks = rk.scatter_cells(case, a)
    assert sum(b.size for b in blocks) == a.size
    assert np.array_equal(rk.gather_cells(case, blocks), a)
    for ax in range(3):
        f = rng.uniform(-1, 1, case.fshape[ax])
        fb = rk.scatter_faces(case, f, ax)
        assert sum(b.size for b in fb) == f.size
        assert np.array_equal(rk.gather_faces(case, fb, ax), f)


@pytest.mark.parametrize("case", CASES, ids=rk.case_id)
def test_wire_count_from_geometry(case):
    """one plane where the stages ship two: the messages of wire_phi, half its bytes; the calls are sums of exchanges"""
    s = irk.STAGES
    for r in range(case.size):
        m, b = rk.wire_phi(case, r)
        assert b % 2 == 0 and irk.wire_exchange(case, r) == (m, b // 2) and m >= 1
        one = irk.wire_exchange(case, r)
        assert irk.wire_apply(case, r) == (1,) + one
        assert irk.wire_solve(case, r, 0) == (0, 0, 0) and irk.wire_solve(case, r, 46) == (46, 46 * one[0], 46 * one[1])
        ms, bs = rk.wire_step(case, r, s)
        assert irk.wire_explicit_step(case, r, s) == (s + 1, ms, bs)
        assert irk.wire_imex(case, r, s, 0, 1.0) == (s + 1, ms, bs)
        assert irk.wire_imex(case, r, s, 10, 1.0) == (s + 11, ms + 10 * one[0], bs + 10 * one[1])
        assert irk.wire_imex(case, r, s, 10, 0.5) == (s + 12, ms + 11 * one[0], bs + 11 * one[1])


def cheb_plan(capi, n):
    import ctypes as C
    f = capi.lib.fldbg_scalar_cheb_plan
    f.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int]
    out = (C.c_int * 5)()
    assert f(*n, out, 5) == 5
    return dict(zip(("per_xcd", "nseg", "band", "fixed_seg", "items"), out))


def test_the_launch_plans_of_the_two_large_blocks(capi):
    """host arithmetic (fldbg_scalar_cheb_plan).  The block of (65, 64, 80) on 1 x 1 x 2 keeps one x segment per wave, but with 8 waves a SIMD the cap of
    k_scalar_cheb is 256 blocks per XCD and that block takes 160: the case stays, and CAP_BLOCK is the one at the cap -- the plan of the 512 x 512 x 256 block that
    tools/scalar_implicit_bench.py --ring times -- with more row segments than waves."""
    big, plan, cap = cheb_plan(capi, (512, 512, 256)), cheb_plan(capi, irk.PLAN_BLOCK), cheb_plan(capi, irk.CAP_BLOCK)
    assert (big["per_xcd"], big["fixed_seg"]) == (256, 1)
    assert (plan["per_xcd"], plan["fixed_seg"], plan["nseg"]) == (160, 1, 2)
    assert (cap["per_xcd"], cap["fixed_seg"], cap["nseg"]) == (256, 1, 2) and cap["items"] > 4 * 8 * cap["per_xcd"]
    smaller = cheb_plan(capi, (65, 64, 64))
    assert not smaller["items"] > 4 * 8 * smaller["per_xcd"]


def test_wire_of_two_known_cases():
    c = rk.Case((7, 5, 6), (2, 1, 1), "channel", own=[(5, 2), (5,), (6,)])
    assert irk.wire_exchange(c, 0) == irk.wire_exchange(c, 1) == (1, 8 * 30)
    p = rk.Case((4, 4, 4), (1, 1, 2), "periodic")
    assert irk.wire_exchange(p, 0) == (2, 2 * 8 * 16)                   # both planes to the same peer
    # the wire DESIGN.md states for a 512^3 block: one plane of 8-byte cells per rank face = 2 MiB
    assert 8 * 512 * 512 == 2 * 2 ** 20


def test_inputs_reach_the_numbers_they_are_made_for():
    from tests import scalar_cases as sc
    from tests import scalar_implicit_reference as ir
    from tests import scalar_reference as sr
    n, bc, uniform = irk.CHANNEL_222[0], irk.CHANNEL_222[2], irk.CHANNEL_222[3]
    I = irk.inputs(n, bc, uniform)
    Pr = sc.problem(n, uniform, bc)
    cfl = sr.cfl(ir.with_gamma(Pr, I["gamma"]), I["V"], I["dt"])
    assert abs(cfl[0] - irk.COURANT) <= 1e-12 and abs(cfl[1] - irk.DIFFUSIVE) <= 1e-10
    assert cfl[1] > irk.STAGES - 1                                       # beyond the explicit limit of the s-stage step
    assert abs(ir.S_of(Pr, I["c_solve"]) - irk.S_SOLVE) <= 1e-12 * irk.S_SOLVE
    k, Bk = ir.steps(*ir.interval(Pr, I["c_solve"]), irk.RTOL, irk.MAXIT)
    assert k > 2 and k % 2 == 0 and Bk <= irk.RTOL
