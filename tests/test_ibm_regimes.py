"""CPU: the marker sets of tests/ibm_regimes.py reach the regimes they name, and the oracle's fo_ibm_interp / fo_ibm_spread agree with the
independent long-double restatement of the spec in tests/ibm_reference.py on every one of them.

The bound is derived, not tuned (u = 2^-53).  The cell-centre index s of a marker carries an absolute error of at most 5 u (n + 2) in double:
h = (x_n - x_0) / n is rounded twice, then one subtraction, one division and the -1/2, each relative u on a number of size <= n + 2 (a stretched axis:
two subtractions of stored centres, one division, one addition to the interval number -- fewer).  |phi'| <= 1 for both delta functions and phi itself
is evaluated with a handful of roundings, so a 1-D weight is off by at most 5 u (n + 2) + 6 u; the weights of the other two axes sum to 1, three axes
and up to four weights each give 60 u (n + 2) max|u|, and the product and the sum of 64 terms stay below 70 u max|u|:

    |U - U_ref| <= u (60 (max_d n_d + 2) + 70) max_support |u|            per marker and component, K = 60 (max n + 2) + 70

(on a marker exactly on a face or a centre, double and long double may start the support one cell apart: the weight that one of them drops is
phi(2 - eps) or phi(1.5 - eps) = O(eps^2) for Peskin, O(eps) for Roma, eps <= 5 u (n + 2) -- inside the same bound, which the lattice set asserts).
Spreading, per cell and component, with B = sum_l |F_l| dV_l / V_cell over the m markers that reach the cell: the same weight error times B, and the
oracle's m additions into f, each rounding a partial sum of size <= |f0| + B:

    |f - f_ref| <= u (K B + (m + 1) (|f0| + B))

A formula error is of order 1e-3; the slack costs nothing.  Measured here, the oracle against the reference (max over markers / cells, components
and boundary types; interp in units of u max_support|u|, to be held against K; spread as a fraction of its bound), Peskin / Roma:

    set              interp [u max|u|]   K        spread [of the bound]
    dense_shell      47.0 / 123.6        16030    0.030  / 0.108
    scan_exact       2.1 / 1.7           7870     0.134  / 0.163
    scan_ragged      35.3 / 95.7         8290     0.112  / 0.078
    dense_stretched  7.6 / 18.0          3070     0.157  / 0.143
    lattice          1.0 / 2.0           1630     0.0007 / 0.0026
    stray            1.1 / 1.3           4030     0.331  / 0.262
    stray_1          0.5 / 0.2           4030     0.0026 / 0.0024
    stray_63         1.1 / 1.3           4030     0.324  / 0.241
    dense_face       1.9 / 2.0           2110     0.016  / 0.017

(the spread figures near 0.1 - 0.3 are cells that a marker reaches with a tiny weight: there the bound is the rounding of f0 + something small.)
"""
import numpy as np
import pytest

from oracle import fluca_oracle as fo
from tests import ibm_reference as ref
from tests import ibm_regimes as R

U_ = 2.0 ** -53
KINDS = [0, 1]
CASES = [(r, bc) for r in R.REGIMES for bc in r.bcs]
IDS = [f"{r.name}-{R.BCNAME[tuple(bc)]}" for r, bc in CASES]


def fields_of(r, kind):
    if r.ranks == (1, 1, 1):
        return R.fields(r, kind)
    # two z ranks: the fuller of the two blocks' bins (own + ghost markers: every marker with a support cell in the block)
    half = r.n[2] // 2
    both = [R.fields(r, kind, block=((0, 0, lo), (r.n[0], r.n[1], half))) for lo in (0, half)]
    return max(both, key=lambda f: f["max_bin"])


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("r", R.REGIMES, ids=[r.name for r in R.REGIMES])
def test_every_set_reaches_the_regime_it_names(r, kind):
    R.check_reach(r, kind, fields_of(r, kind))


def test_the_sets_together_cover_the_untested_paths():
    """k_ibm_spread's third chunk, k_ibm_scan's carry over at least three rounds, the loop that ends on a full round, idle wavefronts in k_ibm_interp"""
    got = [fields_of(r, kind) for r in R.REGIMES for kind in KINDS]
    assert max(f["max_bin"] for f in got) > 512
    assert len(set().union(*[f["scan_rounds"] for f in got])) >= 3
    assert any(f["ntiles"] == 4096 for f in got)
    assert any(f["L_mod_4"] != 0 for f in got)
    assert {f["L_mod_4"] for f in got} >= {1, 3}
    # and the stray set holds what its groups say: nothing of a beyond-walls marker is inside, on either boundary types
    g = R.stray_groups(R.STRAY)
    X = R.STRAY.markers()
    for bc in R.STRAY.bcs:
        per = R.STRAY.periodic(bc)
        gone = np.ones(X[0].size, dtype=bool)
        inside = np.ones(X[0].size, dtype=bool)
        for d in range(3):
            cells, _ = ref.support_1d(0, R.STRAY.xf[d], per[d], X[d])
            inside &= (cells >= 0).any(axis=1)
        gone = ~inside
        walls = g["beyond_walls"].reshape(3, 4)                # per axis: low end by 3 and 40 cells, high end by 3 and 40
        assert all(gone[walls[d]].all() for d in range(3) if not per[d]) and not gone[g["inside"]].any()
        if per[0]:
            assert not gone[np.concatenate([g["one_period"], g["two_periods"], g["far"], g["one_period_back"]])].any()
        else:
            assert gone[np.concatenate([g["one_period"], g["two_periods"], g["far"]])].all()
    assert X[0].size == 67 and all(67 % p for p in range(2, 9))


def data(r, seed=21):
    """the fields and forces every comparison on a set uses: u, f0 (3, ncell), F (3, L), dV (L)"""
    rng = np.random.default_rng(seed)
    L, ncell = r.markers()[0].size, r.n[0] * r.n[1] * r.n[2]
    hvol = np.prod([(r.xf[d][-1] - r.xf[d][0]) / r.n[d] for d in range(3)])
    return dict(u=rng.standard_normal((3, ncell)), F=rng.standard_normal((3, L)), dV=rng.uniform(0.5, 1.5, L) * hvol, f0=rng.standard_normal((3, ncell)))


def interp_excess(r, bc, kind, X, u, U):
    """max over markers and components of |U - U_ref| in units of u max_support|u|, and the bound K"""
    Ur, A, M = ref.interp(r.n, r.xf, r.periodic(bc), kind, X, u)
    err = np.abs(np.asarray(U, dtype=ref.LD).reshape(Ur.shape) - Ur).astype(np.float64)
    assert np.all(err[M == 0.0] == 0.0)                      # no support cell inside: exactly nothing
    return float((err[M > 0] / (U_ * M[M > 0])).max()) if (M > 0).any() else 0.0, ref.ulp_factor(r.n)


def spread_excess(r, bc, kind, X, dV, F, f0, f):
    """max over the reached cells of |f - f_ref| / (u (K B + (m + 1)(|f0| + B))) (<= 1 is the bound), the error in units of u B, and whether
    every other cell still holds f0's bits"""
    K = ref.ulp_factor(r.n)
    cells, add, B, m = ref.spread(r.n, r.xf, r.periodic(bc), kind, X, dV, F)
    f, f0 = f.reshape(F.shape[0], -1), f0.reshape(F.shape[0], -1)
    untouched = np.ones(f.shape[1], dtype=bool)
    untouched[cells] = False
    same = bool(np.array_equal(f[:, untouched], f0[:, untouched]))
    if cells.size == 0:
        return 0.0, 0.0, same
    err = np.abs(f[:, cells].astype(ref.LD) - (f0[:, cells].astype(ref.LD) + add)).astype(np.float64)
    tol = U_ * (K * B + (m[None, :] + 1) * (np.abs(f0[:, cells]) + B))
    return float((err / tol).max()), float((err / (U_ * B)).max()), same


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("r,bc", CASES, ids=IDS)
def test_oracle_matches_the_long_double_reference(r, bc, kind):
    g = fo.Grid(r.n, r.xf, bc, 1e-3)
    X, d = r.markers(), data(r)
    U = g.ibm_interp(kind, X, d["u"])
    ex, K = interp_excess(r, bc, kind, X, d["u"], U)
    f = g.ibm_spread(kind, X, d["dV"], d["F"], d["f0"].copy())
    rel, inB, same = spread_excess(r, bc, kind, X, d["dV"], d["F"], d["f0"], f)
    print(f"{r.name} {R.BCNAME[tuple(bc)]} kind {kind}: interp {ex:.1f} u max|u| (K = {K}), spread {inB:.1f} u B, {rel:.2e} of its bound")
    assert ex <= K, (ex, K)
    assert rel <= 1.0, rel
    assert same
