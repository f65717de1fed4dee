"""CPU-only: the passive-scalar surface of the C host mirror (include/fluca_host.h) as far as it goes without a GPU -- options and the errors that
are detected before any GPU work."""
import ctypes as C

import pytest

P = C.c_void_p


@pytest.fixture(scope="module")
def H():
    from fluca_amd import build
    build.build()
    from fluca_amd import hostapi
    return hostapi


def new_ns(H):
    ns = P()
    assert H.lib.NSCreate(C.byref(ns)) == 0 and H.lib.NSSetType(ns, b"cnlinear") == 0
    return ns


def test_scalar_options(H):
    ns = new_ns(H)
    for name in ("superbee", "minmod", "mc", "vanleer", "vanalbada", "barthjesperson", "venkatakrishnan", "koren", "upwind", "sou", "quick"):
        argc, av = H.argv("-ns_scalar_limiter", name, "-ns_scalar_stages", 3)
        assert H.lib.NSSetFromOptions(ns, argc, av) == 0
    for bad in ("van_leer", "Superbee", "none"):
        argc, av = H.argv("-ns_scalar_limiter", bad)
        assert H.lib.NSSetFromOptions(ns, argc, av) == H.ERR_ARG_UNKNOWN_TYPE
    for bad in (1, 0, -5):
        argc, av = H.argv("-ns_scalar_stages", bad)
        assert H.lib.NSSetFromOptions(ns, argc, av) == H.ERR_ARG_OUTOFRANGE
    H.lib.NSDestroy(C.byref(ns))


def test_scalar_calls_before_setup_and_on_null(H):
    ns = new_ns(H)
    sid, ptr, out = C.c_int(-1), P(), (C.c_double * 2)()
    assert H.lib.NSAddScalar(None, b"dye", 0.0, None, C.byref(sid)) == H.ERR_ARG_NULL
    assert H.lib.NSAddScalar(ns, None, 0.0, None, C.byref(sid)) == H.ERR_ARG_NULL
    assert H.lib.NSAddScalar(ns, b"dye", 0.0, None, None) == H.ERR_ARG_NULL
    assert H.lib.NSAddScalar(ns, b"dye", 0.0, None, C.byref(sid)) == H.ERR_ARG_WRONGSTATE and sid.value == -1      # before NSSetUp
    assert H.lib.NSSetScalarBoundaryCondition(None, 0, 0, 0, 1.0) == H.ERR_ARG_NULL
    assert H.lib.NSSetScalarBoundaryCondition(ns, 0, 0, 0, 1.0) == H.ERR_ARG_WRONGSTATE
    assert H.lib.NSSetScalarSource(None, 0, None) == H.ERR_ARG_NULL and H.lib.NSSetScalarSource(ns, 0, None) == H.ERR_ARG_WRONGSTATE
    assert H.lib.NSSetScalarSubsteps(None, 0, 2) == H.ERR_ARG_NULL and H.lib.NSSetScalarSubsteps(ns, 0, 2) == H.ERR_ARG_WRONGSTATE
    assert H.lib.NSGetScalarArray(ns, 0, None) == H.ERR_ARG_NULL and H.lib.NSGetScalarArray(ns, 0, C.byref(ptr)) == H.ERR_ARG_WRONGSTATE
    assert H.lib.NSGetScalarCFL(ns, 0, None) == H.ERR_ARG_NULL and H.lib.NSGetScalarCFL(ns, 0, out) == H.ERR_ARG_WRONGSTATE
    H.lib.NSDestroy(C.byref(ns))
