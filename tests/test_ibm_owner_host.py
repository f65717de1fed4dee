"""CPU-only: the host-side pieces of the owner-rank IBM markers -- the neighbour of a block across an edge or a corner, argument checks that
never reach the GPU, and the host mirror's option.  The GPU side is tests/test_gpu_ibm_owner.py."""
import ctypes as C
import itertools

import pytest


@pytest.fixture(scope="module")
def capi():
    from fluca_amd import build
    build.build()
    from fluca_amd import capi
    return capi


def test_neighbour_across_edges_and_corners(capi):
    n, ranks = (C.c_int64 * 3)(12, 12, 12), (C.c_int * 3)(3, 2, 2)
    off = lambda *o: (C.c_int * 3)(*o)
    for rank, per in itertools.product(range(12), [(0, 0, 0), (1, 1, 1), (0, 0, 1)]):
        d = capi.fl_decomp()
        assert capi.lib.fl_decomp_default(n, ranks, rank, C.byref(d)) == 0
        p = (C.c_int * 3)(*per)
        assert capi.lib.fl_decomp_neighbor_offset(C.byref(d), p, off(0, 0, 0)) == rank
        for b in range(6):      # a face offset is fl_decomp_neighbor
            o = [0, 0, 0]
            o[b // 2] = 1 if b % 2 else -1
            assert capi.lib.fl_decomp_neighbor_offset(C.byref(d), p, off(*o)) == capi.lib.fl_decomp_neighbor(C.byref(d), p, b)
        for o in itertools.product((-1, 0, 1), repeat=3):
            c, want = [d.coord[a] + o[a] for a in range(3)], None
            for a in range(3):
                if not 0 <= c[a] < ranks[a]:
                    if not per[a]:
                        want = -1
                    c[a] %= ranks[a]
            if want is None:
                want = (c[2] * ranks[1] + c[1]) * ranks[0] + c[0]      # x fastest, as DMStag numbers its ranks
            assert capi.lib.fl_decomp_neighbor_offset(C.byref(d), p, off(*o)) == want, (rank, per, o)
    assert capi.lib.fl_decomp_neighbor_offset(C.byref(d), p, off(2, 0, 0)) == -1
    assert capi.lib.fl_decomp_neighbor_offset(None, p, off(0, 0, 0)) == -1


def test_owned_entry_points_reject_null_handles(capi):
    cnt, out5, m = C.c_int64(), (C.c_int64 * 5)(), C.c_void_p()
    assert capi.lib.fl_ibm_owned_select(None, 0, 1, None, None, None, None, C.byref(cnt)) == -85      # FL_ERR_ARG_NULL
    assert capi.lib.fl_ibm_create_owned(None, 0, 0, None, None, None, None, C.byref(m)) == -85
    assert capi.lib.fl_ibm_owned_counts(None, out5) == -85
    assert capi.lib.fl_ibm_update(None, None, None, None) == -85


def test_marker_distribution_option(capi):
    from fluca_amd import hostapi as H
    ns = C.c_void_p()
    assert H.lib.NSCreate(C.byref(ns)) == 0
    for value, rc in (("owner", 0), ("replicated", 0), ("scattered", H.ERR_ARG_UNKNOWN_TYPE)):
        argc, av = H.argv("-ns_ibm_marker_distribution", value)
        assert H.lib.NSSetFromOptions(ns, argc, av) == rc, value
    H.lib.NSDestroy(C.byref(ns))
