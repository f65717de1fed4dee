"""The table of tests/ksp_stops.py against the oracle (no GPU): every case stops in the oracle for the reason and at the iteration the table
records, a stop by threshold is decided by the recorded margin, a stop with x-updates owed is at no multiple of a ring depth, and every reason
the table claims to reach is reached.  This is what keeps a case of tests/test_gpu_ksp_stops.py from passing by accident: the oracle alone has
to satisfy it."""
import numpy as np
import pytest

from tests import ksp_stops as ks


def _ids(cs):
    return [c.name for c in cs]


ORACLE_CASES = [c for c in ks.STOPS if c.oracle]


@pytest.mark.parametrize("part", sorted({c.part for c in ORACLE_CASES}))
def test_oracle_stops_where_the_table_says(part):
    for c in (c for c in ORACLE_CASES if c.part == part):
        x, info = ks.oracle_solve(c)
        assert (info["reason"], info["iters"]) == (c.reason, c.iters), (c, info["reason"], info["iters"])
        assert len(info["history"]) == c.iters + 1
        if part == "A":
            h0 = info["history"][0]
            if c.rhs[0] == "zero":
                assert h0 == 0.0 and not x.any(), c
            elif len(c.rhs) > 1:
                assert not np.isfinite(h0), c
            elif c.opts.get("norm_type") == ks.NONORM and c.handle == "poisson":
                assert h0 == 0.0, c                           # no norm is formed
            else:
                assert np.isfinite(h0) and h0 > 0.0, c
                if "atol" in c.name:
                    assert h0 < c.opts["atol"], c
            # the oracle's Chebyshev hands back its first step at iteration 0; every other solver the zero guess, which is what the library must
            # return from all of them (tests/test_gpu_ksp_stops.py)
            if c.opts["type"] != ks.CHEB and len(c.rhs) == 1:
                assert not x.any(), c


def test_mg_cases_follow_the_rule_of_their_part():
    """no oracle restates MG-PCG at these stops: the expected reasons are those of the Jacobi-PCG cases, case by case"""
    mg = [c for c in ks.STOPS if not c.oracle]
    assert mg and all(c.part == "A" and c.opts["pc"] == ks.MG for c in mg)
    for c in mg:
        twin = ks.STOP[c.name.replace("A-mg-", "A-cg-jacobi-pre-")]
        assert (c.reason, c.iters, c.rhs) == (twin.reason, twin.iters, twin.rhs), c


THRESHOLD_CASES = [c for c in ks.STOPS if c.threshold is not None]


@pytest.mark.parametrize("c", THRESHOLD_CASES, ids=_ids(THRESHOLD_CASES))
def test_threshold_stops_are_decided_by_the_recorded_margin(c):
    which, value, k = c.threshold
    assert k == c.iters and k >= 1
    x, info = ks.oracle_solve(c)
    h = info["history"]
    if which == "guess-rtol":      # the relative test of a solve from a guess refers to || M b ||, which the oracle reports as rnorm0
        lo, hi = value * info["rnorm0"] / h[k], h[k - 1] / (value * info["rnorm0"])
    else:
        lo, hi = ks.margins(c, h)
    need = ks.MARGIN if c.part == "C" else ks.B_MARGIN
    assert lo >= need and hi >= need, (c, lo, hi)
    if c.reason == ks.ATOL:
        assert info["rnorm"] < c.opts["atol"]
    if c.part == "C" and c.threshold[1] != 1e5:      # dtol is the geometric mean of the two straddling ratios
        assert abs(lo / hi - 1.0) <= 1e-4, (c, lo, hi)
    if c.part == "B":                                 # about half-way of the solve that runs to its relative tolerance
        twin = ks.STOP[c.name.replace("-atol", "-rtol")]
        assert c.reason != ks.ATOL or abs(2 * k - twin.iters) <= 2, (c, k, twin.iters)


RING_CASES = ks.ring_cases()


def test_ring_stops_leave_updates_owed():
    assert len(RING_CASES) >= 4
    for c in RING_CASES:
        owed = [c.iters % d for d in ks.RING_DEPTHS]
        # F-cg stops after 20 iterations: nothing owed at depth 2, four at depth 8 (the default) and at depth 16
        assert all(owed) or (c.name == "F-cg" and owed[1:] == [4, 4]), (c, owed)
        assert "check_every" not in c.opts and c.iters % 16 != 0        # the default polling window: queued launches follow the stop


DIVERGING = [c for c in ks.cases("C") + ks.cases("F")]


@pytest.mark.parametrize("c", DIVERGING, ids=_ids(DIVERGING))
def test_recorded_noise_of_x_at_a_diverging_stop(c):
    """the tolerance of x is X_NOISE_FACTOR times the recorded noise: the oracle's answer to a 1e-16 perturbation of b must still be what was
    recorded (to the digit it was rounded up to), and small enough to leave the comparison a meaning"""
    noise = ks.x_noise(c)
    assert 0.0 < noise <= c.xtol, (c, noise, c.xtol)
    assert c.xtol <= 4.0 * noise or c.xtol <= 1e-14, (c, noise, c.xtol)
    assert ks.X_NOISE_FACTOR * c.xtol <= 2e-9


@pytest.mark.parametrize("c", ks.cases("F"), ids=_ids(ks.cases("F")))
def test_indefinite_matrix_cases_have_their_margin(c):
    k, rel = ks.indefinite_margin(c)
    assert k == c.iters and rel < -ks.F_MARGIN, (c, k, rel)


def test_every_reason_the_table_claims_is_reached():
    reached = {c.reason for c in ORACLE_CASES}
    assert reached == set(ks.REACHED), reached
    assert not reached & set(ks.UNREACHED)
    fams = {(c.handle, c.opts["type"], bool(c.opts.get("cg_single_reduction")), c.opts["pc"] == ks.MG) for c in ks.cases("A")}
    assert len(fams) == 8       # Poisson: CG, single-reduction CG, MG-PCG, BiCGStab, Chebyshev; momentum: BiCGStab, GMRES, Chebyshev


def test_part_D_interval_is_the_default_one():
    """the oracle runs part D on fl_momentum_chebyshev_interval's rule; at the diverging weights the diagonal of A changes sign"""
    for c in ks.cases("D"):
        A = ks.momentum_A(c.n, c.weight)
        emin, emax = ks.momentum_interval(A)
        assert 0.0 < emin < emax
        assert (A.diag().min() < 0.0) == (c.reason == ks.DIV_DTOL), c


def test_overflow_reaches_nanorinf_in_mid_solve():
    """what tests/test_gpu_ksp_stops.py poisons a handle with in mid-solve: the diverging Chebyshev on 1e150 b ends with DIVERGED_NANORINF after a few steps"""
    c = ks.STOP["C-cheb-half"]
    reason, iters = ks.overflow_stop(c, 1e150, 1e300)
    assert reason == ks.DIV_NANORINF and 2 <= iters < c.iters, (reason, iters)
