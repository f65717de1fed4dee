"""The passive scalar on several ranks, without a GPU: the entry point is declared and bound, the scatter / gather helpers of
tests/scalar_ranks.py are each other's inverse on cells and faces for every case of the GPU tests (uneven ownership and periodic axes among
them), and the geometry count of the wire that the GPU tests compare the transport's counters with."""
import os
import re

import numpy as np
import pytest

from tests import scalar_ranks as rk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_create_ranks_is_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "fluca_hip.h")).read()
    assert re.search(r"int fl_scalar_create_ranks\(fl_poisson \*grid_from, const int bc\[6\], fl_scalar \*\*out\);", hdr)
    assert re.search(r"int fl_scalar_create\(fl_poisson \*grid_from, const int bc\[6\], fl_scalar \*\*out\);", hdr)
    src = open(os.path.join(ROOT, "fluca_amd", "capi.py")).read()
    assert '"fl_scalar_create_ranks": (C.c_int, [_P, C.POINTER(C.c_int), C.POINTER(_P)])' in src
    host = open(os.path.join(ROOT, "fluca_amd", "host", "fluca_host.c")).read()
    assert "fl_scalar_create_ranks(ns->poisson" in host


@pytest.mark.parametrize("case", rk.rhs_cases(), ids=rk.case_id)
def test_scatter_then_gather_is_the_identity(case):
    rng = np.random.default_rng(5)
    a = rng.uniform(-1, 1, case.shp)
    blocks = rk.scatter_cells(case, a)
    assert sum(b.size for b in blocks) == a.size                       # every cell owned once
    assert np.array_equal(rk.gather_cells(case, blocks), a)
    for ax in range(3):
        f = rng.uniform(-1, 1, case.fshape[ax])
        fb = rk.scatter_faces(case, f, ax)
        assert sum(b.size for b in fb) == f.size                       # every face owned once
        assert np.array_equal(rk.gather_faces(case, fb, ax), f)
    for r in range(case.size):
        lo, ln = case.lo_len(r)
        assert blocks[r].shape == (ln[2], ln[1], ln[0])


def test_uneven_and_periodic_ownership():
    c = rk.Case((7, 5, 6), (2, 1, 1), "channel", own=[(5, 2), (5,), (6,)])
    assert [case_len for case_len in (c.lo_len(0), c.lo_len(1))] == [([0, 0, 0], [5, 5, 6]), ([5, 0, 0], [2, 5, 6])]
    # x is not periodic: the last rank owns the face behind its last cell; z is periodic and held alone: no neighbour, no extra face
    assert c.face_slices(0, 0)[2] == slice(0, 5) and c.face_slices(1, 0)[2] == slice(5, 8)
    assert c.neighbours(0) == [False, True, False, False, False, False] and c.neighbours(1) == [True, False, False, False, False, False]
    p = rk.Case((4, 4, 4), (1, 1, 2), "periodic")
    assert p.neighbours(0) == p.neighbours(1) == [False, False, False, False, True, True]       # the same peer behind both ends
    assert p.face_slices(1, 2)[0] == slice(2, 4)


def test_wire_count_from_geometry():
    """two planes of 8-byte cells across every rank face for phi, one plane of faces to the low neighbour for V"""
    c = rk.Case((7, 5, 6), (2, 1, 1), "channel", own=[(5, 2), (5,), (6,)])
    assert rk.wire_phi(c, 0) == rk.wire_phi(c, 1) == (1, 2 * 8 * 30)
    assert rk.wire_velocity(c, 0) == (0, 0) and rk.wire_velocity(c, 1) == (1, 8 * 30)
    assert rk.wire_rhs(c, 1) == (2, 3 * 8 * 30) and rk.wire_step(c, 1, 5) == (6, 11 * 8 * 30)
    p = rk.Case((4, 4, 4), (1, 1, 2), "periodic")
    assert rk.wire_phi(p, 0) == (2, 2 * 2 * 8 * 16) and rk.wire_velocity(p, 0) == (1, 8 * 16)
    e = rk.Case((7, 6, 5), (2, 2, 2), "channel", uniform=False)
    for r in range(8):
        lo, ln = e.lo_len(r)
        nb = e.neighbours(r)
        assert sum(nb) == 4                                          # one neighbour along x and y, the same peer behind both ends of the periodic z
        assert rk.wire_phi(e, r) == (4, 16 * (ln[1] * ln[2] + ln[0] * ln[2] + 2 * ln[0] * ln[1]))
    # the wire cost DESIGN.md states for a 512^3 block: 2 planes x 8 B per rank face = 4 MiB
    assert 2 * 8 * 512 * 512 == 4 * 2 ** 20
