"""No GPU: what fl_ibm_force (include/fluca_hip.h) and NSGetImmersedBoundaryForce / NSSetImmersedBoundaryBodies / NSMonitorImmersedBoundaryForce
(include/fluca_host.h) answer before any device work, and the arithmetic of the order-independent sum in its numpy restatement
(tests/ibm_force_reference.py): identical bits under permutations and under any split into "ranks", and the error against the exact rational sum
within L 2^(E-61) + 1/2 ulp on inputs chosen to hurt.  The kernels themselves: tests/test_gpu_ibm_force.py."""
import ctypes as C
import math
from fractions import Fraction

import numpy as np
import pytest

from tests import ibm_force_reference as fr


def test_calls_without_a_set_are_argument_errors():
    from fluca_amd import capi
    lib = capi.lib
    about, force, torque = (C.c_double * 3)(), (C.c_double * 3)(7., 7., 7.), (C.c_double * 3)(7., 7., 7.)
    assert lib.fl_ibm_force(None, None, None, None, 1, about, force, torque) == -85          # FL_ERR_ARG_NULL
    assert lib.fl_ibm_force(None, None, None, None, 0, None, None, None) == -85
    assert list(force) == [7.] * 3 and list(torque) == [7.] * 3


def test_the_host_calls_need_a_solver_with_an_immersed_boundary():
    from fluca_amd import hostapi as H
    f, t = (C.c_double * 3)(7., 7., 7.), (C.c_double * 3)(7., 7., 7.)
    assert H.lib.NSGetImmersedBoundaryForce(None, None, f, t) == H.ERR_ARG_NULL
    assert H.lib.NSSetImmersedBoundaryBodies(None, 1, None) == H.ERR_ARG_NULL
    assert H.lib.NSMonitorImmersedBoundaryForce(None, None) == H.ERR_ARG_NULL
    ns = C.c_void_p()
    assert H.lib.NSCreate(C.byref(ns)) == 0
    assert H.lib.NSGetImmersedBoundaryForce(ns, None, None, t) == H.ERR_ARG_NULL
    assert H.lib.NSGetImmersedBoundaryForce(ns, None, f, t) == H.ERR_ARG_WRONGSTATE             # no immersed boundary, no step
    assert H.lib.NSSetImmersedBoundaryBodies(ns, 2, None) == H.ERR_ARG_WRONGSTATE
    assert H.lib.NSSetImmersedBoundaryBodies(ns, 0, None) == H.ERR_ARG_OUTOFRANGE
    assert H.lib.NSSetImmersedBoundaryBodies(ns, 65, None) == H.ERR_ARG_OUTOFRANGE
    assert list(f) == [7.] * 3 and list(t) == [7.] * 3
    H.lib.NSDestroy(C.byref(ns))


# ------------------------------------------------------------------------------------------------ the split sum in numpy

def _hurting_inputs():
    rng = np.random.default_rng(20261018)
    L = 4097
    spread = rng.standard_normal(L) * np.exp2(rng.uniform(-60, 0, L))              # magnitudes over 2^60
    big = rng.standard_normal(L // 2) * 1e6
    cancel = np.concatenate([big, -big, rng.standard_normal(1) * 1e-9])           # near-total cancellation: the sum is 1e-15 of the terms
    dominant = np.concatenate([[1.2345678901234567e12], rng.standard_normal(L - 1) * 1e-3])
    return {"spread over 2^60": spread, "cancellation": cancel, "one dominant term": dominant, "all equal": np.full(L, 0.1),
            "L = 1": np.array([-math.pi]), "L = 65": rng.standard_normal(65)}


@pytest.mark.parametrize("name", list(_hurting_inputs()))
def test_the_split_sum_stays_within_its_bound(name):
    t = _hurting_inputs()[name]
    E = fr.group_exponent(t)
    got = float(fr.split_sum(t, E))
    err, bd = abs(Fraction(got) - fr.exact_sum(t)), fr.bound(t.size, E, got)
    print(f"{name}: L {t.size} E {E} error {float(err):.3e} bound {float(bd):.3e}")
    assert err <= bd
    # the parts are what the header says: integer multiples of u1 / u2 below 2^30 in size, the tail at most 2^(E-61)
    hi, mid = fr.split(t, E)
    a, b = hi / math.ldexp(1.0, E - 30), mid / math.ldexp(1.0, E - 60)
    assert np.array_equal(a, np.rint(a)) and np.array_equal(b, np.rint(b)) and np.abs(a).max() <= 2.0 ** 30 and np.abs(b).max() <= 2.0 ** 29
    assert np.abs((t - hi) - mid).max() <= math.ldexp(1.0, E - 61)


@pytest.mark.parametrize("name", list(_hurting_inputs()))
def test_the_split_sum_has_the_same_bits_in_any_order_and_over_any_ranks(name):
    t = _hurting_inputs()[name]
    E = fr.group_exponent(t)
    want = float(fr.split_sum(t, E))
    rng = np.random.default_rng(3)
    for _ in range(5):
        p = rng.permutation(t)
        assert float(fr.split_sum(p, E)) == want
        assert float(np.add.reduce(fr.split(p, E)[0]) + np.add.reduce(fr.split(p, E)[1])) == want
        hi, mid = fr.split(p, E)
        assert math.fsum(hi) + math.fsum(mid) == want                             # the parts add up EXACTLY: any order is the exact one
        cuts = np.sort(rng.integers(0, t.size + 1, 7))
        assert float(fr.split_sum_parts(np.split(p, cuts), E)) == want              # eight "ranks", some of them empty
    # a plain floating-point sum does depend on the order, on the inputs where that can show at all (no claim for constant or single terms)
    if name in ("spread over 2^60", "cancellation"):
        assert len({float(np.sum(rng.permutation(t))) for _ in range(20)}) > 1


def test_the_terms_round_once_per_operation_and_take_the_minimum_image():
    rng = np.random.default_rng(9)
    L = 50
    X, F, dV = rng.uniform(0, 1, (3, L)), rng.standard_normal((3, L)), rng.uniform(0.5, 1.5, L)
    about = np.array([0.5, 0.5, 0.03125])
    tf, tt = fr.terms(X, F, dV, about, (None, None, 1.0))
    r = X - about[:, None]
    r[2] -= np.rint(r[2])
    assert np.abs(r[2]).max() <= 0.5 and np.array_equal(tf, F * dV)
    for l in range(L):      # scalar Python arithmetic rounds every operation once
        want = ((float(r[1, l]) * float(F[2, l])) - (float(r[2, l]) * float(F[1, l]))) * float(dV[l])
        assert tt[0, l] == want
    ref = fr.reference(X, F, dV, about[None], (None, None, 1.0))
    assert fr.within(ref, "force", ref["force"]) <= 1.0 and fr.within(ref, "torque", ref["torque"]) <= 1.0
