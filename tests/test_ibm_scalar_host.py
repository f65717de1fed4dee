"""No GPU: the scalar forcing on immersed-boundary markers (include/fluca_hip_ibm_scalar.h, NSSetScalarImmersedBoundary) -- the header against the
ctypes table and the exports, the long-double restatement of tests/ibm_scalar_reference.py on its own (one pass is spread(T - interp phi); what the
markers hand out is what the field gains; four passes leave a smaller defect than one on a marker set built for it; the marker set reaches the
regimes the GPU tests name), and the argument errors that return before any device work.  tests/test_gpu_ibm_scalar*.py run the kernels."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import ibm_reference as ref
from tests import ibm_scalar_cases as sc
from tests import ibm_scalar_reference as isr
from tests import stream_order as so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = [0, 1]
BOTH = pytest.mark.parametrize("uniform", [True, False], ids=["uniform", "stretched"])


def header():
    return open(os.path.join(ROOT, "include", "fluca_hip_ibm_scalar.h")).read()


def test_header_table_and_exports_name_the_same_functions():
    from fluca_amd import capi
    decl = so.declarations(header())
    assert sorted(decl) == sorted(capi.PROTOTYPES_IBM_SCALAR) == ["fl_ibm_scalar_force", "fl_ibm_scalar_rate"]
    for name, (params, comment) in decl.items():
        assert hasattr(capi.lib, name), name
        assert len(params) == len(capi.PROTOTYPES_IBM_SCALAR[name][1]), name
        assert comment.strip(), f"{name} has no comment"
    assert not set(capi.PROTOTYPES_IBM_SCALAR) & (set(capi.PROTOTYPES) | set(capi.PROTOTYPES_IMPLICIT))
    main = open(os.path.join(ROOT, "include", "fluca_hip.h")).read()
    assert not re.search(r"fl_ibm_scalar", main) and '#include "fluca_hip.h"' in header()


@pytest.mark.parametrize("kind", KINDS)
@BOTH
def test_the_marker_set_reaches_its_regimes(uniform, kind):
    xf, X = sc.grid(uniform), sc.markers()
    f = ref.regime_fields(sc.N, kind, X, sc.PERIODIC, xf)
    assert 200 <= X[0].size <= 600 and X[0].size % 4 and f["max_bin"] > 256 and any(n % 8 for n in sc.N)
    g = sc.group_slices()
    cz, _ = ref.support_1d(kind, xf[2], True, X[2][g["seam"]])
    assert any(set(row) >= {0, sc.N[2] - 1} for row in cz.tolist())                    # a support on both sides of the periodic seam
    cx, _ = ref.support_1d(kind, xf[0], False, X[0][g["wall"]])
    cy, _ = ref.support_1d(kind, xf[1], False, X[1][g["wall"]])
    assert (cx < 0).any() and (cy < 0).any()                                           # supports cut by the low x and the high y wall
    for d in range(3):                                                                 # the inner groups stay two cells from the walls
        c, _ = ref.support_1d(kind, xf[d], sc.PERIODIC[d], sc.markers(sc.INNER)[d])
        assert (c >= 0).all() and (sc.PERIODIC[d] or (c.min() >= 2 and c.max() <= sc.N[d] - 3))


@pytest.mark.parametrize("kind", KINDS)
@BOTH
def test_one_pass_is_spread_of_the_defect(uniform, kind):
    """against ibm_reference.interp / spread themselves (double fields in, long double out): the first pass starts from a double field"""
    xf, X, d = sc.grid(uniform), sc.markers(), sc.data()
    geo = isr.Geometry(sc.N, xf, sc.PERIODIC, kind, X)
    phi1, Q, qs, _ = isr.force(geo, d["T"], d["dV"], d["phi0"], 1)
    Phi = ref.interp(sc.N, xf, sc.PERIODIC, kind, X, d["phi0"])[0][0]
    q = d["T"].astype(ref.LD) - Phi
    assert np.array_equal(q, qs[0]) and np.array_equal(Q, q)
    # ibm_reference.spread takes a double F: hand it q's double part and remainder
    hi = q.astype(np.float64)
    lo = (q - hi.astype(ref.LD)).astype(np.float64)
    cells, add, _, _ = ref.spread(sc.N, xf, sc.PERIODIC, kind, X, d["dV"], np.stack([hi, lo]))
    want = d["phi0"].astype(ref.LD)
    want[cells] += add[0] + add[1]
    err = np.abs(phi1 - want).astype(np.float64)
    assert err.max() <= 2.0 ** -60 * max(1.0, float(np.abs(want).max()))
    assert np.array_equal(phi1[~geo.reached()], d["phi0"][~geo.reached()].astype(ref.LD))


@pytest.mark.parametrize("npass", sc.NPASSES)
@pytest.mark.parametrize("kind", KINDS)
@BOTH
def test_the_field_gains_what_the_markers_hand_out(uniform, kind, npass):
    """sum_c (phi_out - phi_in)_c vol_c = sum_l Q_l dV_l for markers at least two cells from a non-periodic wall"""
    xf, X, d = sc.grid(uniform), sc.markers(sc.INNER), sc.data(sc.INNER)
    geo = isr.Geometry(sc.N, xf, sc.PERIODIC, kind, X)
    for T in (d["T"], d["Tbody"]):
        phi1, Q, _, _ = isr.force(geo, T, d["dV"], d["phi0"], npass)
        lhs, rhs, margin = sc.conservation(xf, d["phi0"], phi1.astype(np.float64), Q.astype(np.float64), d["dV"])
        assert abs(lhs - rhs) <= margin and abs(rhs) > 1e3 * margin, (lhs, rhs, margin)


@pytest.mark.parametrize("kind", KINDS)
def test_four_passes_leave_a_smaller_defect_than_one(kind):
    """uniform grid, marker spacing about h, dV = h^3"""
    X, dV, T, phi0 = sc.contraction_set()
    geo = isr.Geometry(sc.N, sc.grid(True), sc.PERIODIC, kind, X)
    d1 = isr.defect(geo, T, isr.force(geo, T, dV, phi0, 1)[0])
    d4 = isr.defect(geo, T, isr.force(geo, T, dV, phi0, 4)[0])
    print(f"kind {kind}: defect {isr.defect(geo, T, phi0):.3f} -> {d1:.3f} (1 pass) -> {d4:.3f} (4 passes)")
    assert d4 < d1 < isr.defect(geo, T, phi0)


def test_rate_is_the_split_sum_whatever_the_order():
    from tests import ibm_force_reference as fr
    d = sc.data()
    rng = np.random.default_rng(73)
    Q = rng.standard_normal(d["dV"].size) * 10.0 ** rng.integers(-6, 6, d["dV"].size)
    want = isr.rate(Q, d["dV"], d["body"], 3)
    p = rng.permutation(Q.size)
    assert np.array_equal(want, isr.rate(Q[p], d["dV"][p], d["body"][p], 3))
    t = Q * d["dV"]
    E = fr.group_exponent(t)
    for b in range(3):
        exact = fr.exact_sum(t[d["body"] == b])
        assert abs(exact - fr.Fraction(float(want[b]))) <= fr.bound(Q.size, E, want[b])
    Q[7] = np.inf
    assert np.isnan(isr.rate(Q, d["dV"], d["body"], 3)).all()


def test_calls_without_a_set_are_argument_errors():
    from fluca_amd import capi
    lib = capi.lib
    x = C.c_void_p(4096)                       # never dereferenced: the handle is checked first
    v = (C.c_double * 3)(1.0, 2.0, 3.0)
    assert lib.fl_ibm_scalar_force(None, 1, None, None, 3, v, x, x, x) == -85          # FL_ERR_ARG_NULL
    assert lib.fl_ibm_scalar_force(None, 1, x, None, 1, None, x, x, None) == -85
    assert lib.fl_ibm_scalar_rate(None, x, x, None, 3, v) == -85
    assert list(v) == [1.0, 2.0, 3.0]


def test_the_host_mirror_checks_before_any_device_work():
    from fluca_amd import hostapi as H
    v = (C.c_double * 2)(1.0, 0.0)
    assert H.lib.NSSetScalarImmersedBoundary(None, 0, 1, v) == H.ERR_ARG_NULL
    assert H.lib.NSGetScalarImmersedBoundaryRate(None, 0, v) == H.ERR_ARG_NULL
    ns = C.c_void_p()
    assert H.lib.NSCreate(C.byref(ns)) == 0
    assert H.lib.NSSetScalarImmersedBoundary(ns, 0, 1, v) == H.ERR_ARG_WRONGSTATE      # no immersed boundary
    assert H.lib.NSSetScalarImmersedBoundary(ns, 0, 17, v) == H.ERR_ARG_OUTOFRANGE
    assert H.lib.NSSetScalarImmersedBoundary(ns, 0, -2, v) == H.ERR_ARG_OUTOFRANGE
    assert H.lib.NSGetScalarImmersedBoundaryRate(ns, 0, v) == H.ERR_ARG_WRONGSTATE
    assert list(v) == [1.0, 0.0]
    H.lib.NSDestroy(C.byref(ns))
