"""-m gpu: fl_scalar_boundary_flux (k_scalar_flux, fluca_amd/csrc/fl_scalar.hip) against tests/buoyancy_reference.wall_fluxes in long double.

The bound per boundary and part is derived (buoyancy_reference.wall_fluxes): U sum_f (|V| eF A + 3 |V F A|) for the convective part -- eF the bound
of scalar_reference.axis_terms on the face value, three roundings for V F, the area and their product -- the analogue with Gamma eG for the
diffusive part, and (faces - 1) U sum_f |term| for a sum taken in any order.  The budget ties the twelve numbers to fl_scalar_rhs, which
tests/test_gpu_scalar.py checks cell by cell:  sum_c R(phi)(c) vol(c) = sum_d (flux_lo - flux_hi) + sum_c q vol  to  U sum_c E(c) vol(c) + the flux
bounds.  Grids: 5 x 4 x 3 and 70 x 3 x 9 (a row wider than 64 lanes; planes of 27 to 630 faces: less than a wave to three blocks)."""
import ctypes as C

import numpy as np
import pytest

from tests import buoyancy_reference as br
from tests import scalar_cases as sc
from tests import scalar_ranks as rk
from tests import scalar_reference as sr

pytestmark = pytest.mark.gpu

D, N, P = sr.DIRICHLET, sr.NEUMANN, sr.PERIODIC
GAMMA = 0.0125
U = sr.U
# both ends of all three axes, Dirichlet and Neumann, and periodic axes
BCS = {
    "dirichlet": sc.BC_SETS["dirichlet"],
    "neumann": sc.BC_SETS["neumann"],
    "channel": sc.BC_SETS["channel"],
    "mixed": ((N, D, D, N, N, D), (0.9, -0.4, 0.25, 1.2, -0.8, 0.6)),
    "periodic": sc.BC_SETS["periodic"],
    "x-only": ((D, N, P, P, P, P), (0.7, -0.6, 0.0, 0.0, 0.0, 0.0)),
}
GRIDS = [(5, 4, 3), (70, 3, 9)]


def problem(n, uniform, bcname, gamma=0.0, limiter="superbee"):
    kinds, vals = BCS[bcname]
    return sr.Problem(sc.faces(n, uniform), kinds, vals, gamma=gamma, limiter=limiter)


def random_fields(Pr, seed):
    """phi, V of both signs on every face (inflow and outflow on the boundary faces), q"""
    rng = np.random.default_rng(seed)
    cs, fs = Pr.shapes()
    return rng.uniform(-1.0, 1.0, cs), [rng.uniform(-1.0, 1.0, s) for s in fs], rng.uniform(-1.0, 1.0, cs)


def _dev(a):
    from tests.gpu_common import dev
    return dev(np.ascontiguousarray(a).reshape(-1))


def check_flux(got, Pr, phi, V, what, limiter=None):
    want, bound = br.wall_fluxes(Pr, phi, V, np.longdouble, limiter=limiter)
    err = np.abs(np.asarray(got, dtype=np.longdouble) - want).astype(np.float64)
    tol = br.slack(bound)
    print(f"{what}: largest error / bound = {float((err / tol).max()):.3f}")
    assert (err <= tol).all(), (what, got.tolist(), np.asarray(want, dtype=np.float64).tolist(), (err / tol).tolist())
    for d in range(3):
        if Pr.periodic(d):
            # exactly 0.0, not a small number
            assert np.array_equal(np.asarray(got[2 * d:2 * d + 2]).view(np.int64), np.zeros((2, 2)).view(np.int64)), (what, d)
    return bound


@pytest.mark.parametrize("uniform", [True, False], ids=["uniform", "stretched"])
@pytest.mark.parametrize("bcname", ["dirichlet", "neumann", "channel", "mixed", "periodic"])
@pytest.mark.parametrize("n", GRIDS, ids=lambda n: "x".join(map(str, n)))
def test_flux_and_budget(n, bcname, uniform):
    from fluca_amd.poisson import Poisson
    from fluca_amd.scalar import Scalar
    from tests.gpu_common import host
    kinds, vals = BCS[bcname]
    Pz = Poisson(n, sc.faces(n, uniform), sc.poisson_bc(kinds), 1e-3)
    S = Scalar(Pz, kinds, vals)
    try:
        for limiter, gamma, seed in (("superbee", 0.0, 1), ("vanleer", GAMMA, 2)):
            Pr = problem(n, uniform, bcname, gamma, limiter)
            phi, V, q = random_fields(Pr, seed)
            S.set_limiter(limiter)
            S.set_diffusivity(gamma)
            S.set_velocity(*[_dev(v) for v in V])
            got = S.boundary_flux(_dev(phi))
            assert got.shape == (6, 2)
            again = S.boundary_flux(_dev(phi))
            assert np.array_equal(got.view(np.int64), again.view(np.int64))           # the same bits on every call
            what = f"{n} {'uniform' if uniform else 'stretched'} {bcname} {limiter} gamma={gamma}"
            fb = check_flux(got, Pr, phi, V, what)
            if gamma == 0.0:
                assert (got[:, 1] == 0.0).all()
            else:
                assert all(got[b, 1] != 0.0 for b in range(6) if kinds[b] == D)
            # the budget: fl_scalar_rhs summed on the host in long double against the twelve numbers
            R = host(S.rhs(_dev(phi), _dev(q))).reshape(phi.shape).astype(np.longdouble)
            _, E, _ = sr.rhs(Pr, phi, V, q, np.longdouble, bounds=True)
            vol = sr.volumes(Pr, np.longdouble)
            lhs = (R * vol).sum()
            rhs = br.budget(got.astype(np.longdouble)) + (q.astype(np.longdouble) * vol).sum()
            bound = float(U * (E * vol).sum()) * (1 + 2.0 ** -10) + float(br.slack(fb).sum())
            print(f"budget {what}: |sum R vol - fluxes - sum q vol| / bound = {float(abs(lhs - rhs)) / bound:.3f}")
            assert float(abs(lhs - rhs)) <= bound, (what, float(lhs), float(rhs), bound)
    finally:
        S.close()
        Pz.close()


def test_wrongstate_before_a_velocity_is_set():
    from fluca_amd import capi
    from fluca_amd.poisson import Poisson
    from fluca_amd.scalar import Scalar
    n = (5, 4, 3)
    kinds, vals = BCS["channel"]
    Pz = Poisson(n, sc.faces(n, True), sc.poisson_bc(kinds), 1e-3)
    S = Scalar(Pz, kinds, vals)
    phi = Pz.empty().zero_()
    out = (C.c_double * 12)(*([7.0] * 12))
    assert capi.lib.fl_scalar_boundary_flux(S.h, C.c_void_p(phi.data_ptr()), out) == -73 and list(out) == [7.0] * 12
    with pytest.raises(capi.FlucaError):
        S.boundary_flux(phi)
    S.close()
    Pz.close()


# ---- rank grids in one process

class FluxCase(rk.Case):
    """scalar_ranks.Case with the boundary set of this file"""

    def __init__(self, n, ranks, bcname, uniform=False, own=None, kappa=1e-3):
        self.n, self.ranks, self.bcname, self.uniform, self.kappa = tuple(n), tuple(ranks), bcname, uniform, kappa
        self.kinds, self.vals = BCS[bcname]
        self.own = own if own is not None else [rk.default_split(n[d], ranks[d]) for d in range(3)]
        self.xf = sc.faces(self.n, uniform)
        self.periodic = [self.kinds[2 * d] == P for d in range(3)]
        self.bc = [3 if self.kinds[b] == P else 1 for b in range(6)]
        self.shp = (n[2], n[1], n[0])
        nf = [n[d] if self.periodic[d] else n[d] + 1 for d in range(3)]
        self.fshape = [(n[2], n[1], nf[0]), (n[2], nf[1], n[0]), (nf[2], n[1], n[0])]
        self.size = ranks[0] * ranks[1] * ranks[2]


def _flux_worker(R, case, blocks, limiter, gamma):
    import torch
    from fluca_amd.scalar import Scalar
    from tests.test_gpu_config5 import _handle
    Pz, d, s = _handle(R, case)
    with torch.cuda.stream(s):
        dev = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64).ravel(), device="cuda")
        S = Scalar(Pz, case.kinds, case.vals, limiter=limiter, gamma=gamma)
        phi = dev(blocks["phi"][R.rank])
        out = (C.c_double * 12)()
        from fluca_amd import capi
        assert capi.lib.fl_scalar_boundary_flux(S.h, C.c_void_p(phi.data_ptr()), out) == -73       # before a velocity is set, on every rank
        S.set_velocity(*[dev(blocks["V"][a][R.rank]) for a in range(3)])
        got = S.boundary_flux(phi)
        again = S.boundary_flux(phi)
        s.synchronize()
        S.close()
    Pz.close()
    return got, again


RANK_CASES = [
    FluxCase((4, 5, 4), (2, 1, 1), "channel"),           # blocks of two cells along the split x
    FluxCase((5, 4, 4), (1, 2, 2), "channel"),           # y split, the periodic z split over two ranks: two-cell blocks along both
    FluxCase((4, 4, 4), (2, 2, 2), "channel"),
    FluxCase((4, 4, 4), (2, 2, 2), "mixed"),
    FluxCase((7, 6, 5), (2, 2, 2), "dirichlet"),
    FluxCase((6, 4, 4), (3, 1, 1), "x-only"),            # the middle rank touches no boundary and still takes part
]


@pytest.mark.parametrize("case", RANK_CASES, ids=lambda c: "x".join(map(str, c.n)) + "-" + "x".join(map(str, c.ranks)) + "-" + c.bcname)
def test_rank_grids(case):
    from tests import inproc
    Pr = problem(case.n, case.uniform, case.bcname, GAMMA, "vanleer")
    phi, V, _ = random_fields(Pr, 3)
    if case.ranks == (3, 1, 1):
        assert case.neighbours(1)[:2] == [True, True] and case.periodic[1:] == [True, True]         # rank 1: every end periodic or a rank face
    blocks = {"phi": rk.scatter_cells(case, phi), "V": [rk.scatter_faces(case, V[a], a) for a in range(3)]}
    res = inproc.run_threads(case.size, _flux_worker, case, blocks, "vanleer", GAMMA)
    got = res[0][0]
    for r in range(case.size):
        for a in res[r]:
            assert np.array_equal(a.view(np.int64), got.view(np.int64)), ("every rank and every call return the same bits", r)
    check_flux(got, Pr, phi, V, f"{case.n} on {case.ranks} {case.bcname}")
