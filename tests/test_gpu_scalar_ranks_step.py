"""-m gpu: fl_scalar_step on rank grids (the ranks as threads of one process, tests/inproc.py): every step against the rks2 step of
tests/scalar_reference.py on the GLOBAL grid, started from the gathered state before that step and held to its derived one-step bound (the method
of tests/test_gpu_scalar_step.py); bitwise equality across rank grids -- the fused pack of stage k feeds stage k + 1 exactly what a pack kernel
would; conservation of sum phi vol; boundedness of the TVD limiters across a rank face; the wire per step.  All reference work is done before the
rank threads start or after they end."""
import numpy as np
import pytest

from tests import inproc
from tests import scalar_cases as sc
from tests import scalar_ranks as rk
from tests import scalar_reference as sr

pytestmark = pytest.mark.gpu

ULP1 = 2.0 ** -52
GAMMA = 0.0125
SEQUENCE = [(2, False), (3, True), (5, True)]     # stages, with the source


def _step_worker(R, case, limiter, blocks, dt):
    import torch
    from fluca_amd.scalar import Scalar
    from tests.test_gpu_config5 import _handle
    P, d, s = _handle(R, case)
    states = []
    with torch.cuda.stream(s):
        dev = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64).ravel(), device="cuda")
        S = Scalar(P, case.kinds, case.vals, limiter=limiter, gamma=GAMMA)
        S.set_velocity(*[dev(blocks["V"][a][R.rank]) for a in range(3)])
        qd = dev(blocks["q"][R.rank])
        phid = dev(blocks["phi"][R.rank])
        states.append(phid.cpu().numpy().copy())
        for stages, with_source in SEQUENCE:
            s.synchronize()
            w0 = R.stats()
            S.step(phid, dt, stages, qd if with_source else None)
            s.synchronize()
            w1 = R.stats()
            # s exchanges of the phi slabs (one kernel-packed, s - 1 packed by the stages) and one of V's high faces
            assert (w1["messages"] - w0["messages"], w1["bytes"] - w0["bytes"]) == rk.wire_step(case, R.rank, stages), (R.rank, stages, w0, w1)
            assert w1["exchanges"] - w0["exchanges"] <= stages + 1 and w1["allreduces"] == w0["allreduces"]
            states.append(phid.cpu().numpy().copy())
        S.close()
    P.close()
    return states


def _run_steps(case, limiter, phi0, dt):
    V = sc.velocity(case.n, case.bcname)
    blocks = {"V": [rk.scatter_faces(case, V[a], a) for a in range(3)], "q": rk.scatter_cells(case, sc.source(case.n)), "phi": rk.scatter_cells(case, phi0)}
    res = inproc.run_threads(case.size, _step_worker, case, limiter, blocks, dt)
    return [rk.gather_cells(case, [res[r][a] for r in range(case.size)]) for a in range(len(SEQUENCE) + 1)]


@pytest.mark.parametrize("n,ranks,own,bcname,limiter,other", [((7, 5, 6), (2, 1, 1), [(5, 2), (5,), (6,)], "channel", "superbee", (1, 2, 1)),
                                                              ((4, 4, 4), (1, 1, 2), None, "dirichlet", "koren", (2, 1, 1)),
                                                              ((7, 6, 5), (2, 2, 2), None, "neumann", "venkatakrishnan", (1, 2, 1))],
                         ids=["7x5x6-channel-2x1x1", "4x4x4-dirichlet-1x1x2", "7x6x5-neumann-2x2x2"])
def test_steps_against_rks2_and_across_rank_grids(n, ranks, own, bcname, limiter, other):
    case = rk.Case(n, ranks, bcname, uniform=False, own=own)
    kinds, vals = sc.BC_SETS[bcname]
    Pr = sr.Problem(sc.faces(n, False), kinds, vals, GAMMA, limiter)
    V = sc.velocity(n, bcname)
    q = sc.source(n)
    phi0 = sc.phi_field(n, "random") * 0.5 + sc.phi_field(n, "step")
    adv, dif = sr.cfl(Pr, V, 1.0)
    dt = 0.5 / (adv + dif)
    states = _run_steps(case, limiter, phi0, dt)
    assert np.array_equal(states[0], phi0)
    worst = 0.0
    for (stages, with_source), before, got in zip(SEQUENCE, states[:-1], states[1:]):
        want, B = sr.step(Pr, before, V, dt, stages, q if with_source else None, np.longdouble, bounds=True)
        err = np.abs(got.astype(np.longdouble) - want).astype(np.float64)
        tol = np.asarray(B, dtype=np.float64) * (1 + 2.0 ** -10)
        worst = max(worst, float((err / tol).max()))
        assert (err <= tol).all(), (stages, float(err.max()), float((err / tol).max()), tuple(np.argwhere(err > tol)[0]))
        assert float(np.abs(got - before).max()) > 1e-3          # (the step did something)
    print(f"step {rk.case_id(case)}: largest error / bound = {worst:.3f}")
    # another rank grid: the same bits after every one of the three steps
    again = _run_steps(rk.Case(n, other, bcname, uniform=False), limiter, phi0, dt)
    for a, b in zip(states, again):
        assert np.array_equal(a, b), (other, int((a != b).sum()), float(np.abs(a - b).max()))


def _mass_worker(R, case, blocks, dt, nsteps):
    import torch
    from fluca_amd.scalar import Scalar
    from tests.test_gpu_config5 import _handle
    P, d, s = _handle(R, case)
    with torch.cuda.stream(s):
        dev = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64).ravel(), device="cuda")
        S = Scalar(P, case.kinds, case.vals, limiter="superbee", gamma=0.002)
        S.set_velocity(*[dev(blocks["V"][a][R.rank]) for a in range(3)])
        phid = dev(blocks["phi"][R.rank])
        stats, states = [S.stats(phid)], [phid.cpu().numpy().copy()]
        for _ in range(nsteps):
            S.step(phid, dt, 5)
            states.append(phid.cpu().numpy().copy())
        stats.append(S.stats(phid))
        S.close()
    P.close()
    return stats, states


def test_mass_is_conserved():
    """10 steps, s = 5, in the solenoidal V of tests/test_gpu_scalar_step.py on the periodic box over 2 x 2 x 1 ranks: sum phi vol moves by no more
    than that test's bound -- per step the volume sum of the step's bound, and the two sums' own rounding, here the depth of a rank's sum plus one
    rounding per rank for the all-reduce"""
    from tests.test_gpu_scalar_step import BOX_GRID, solenoidal
    n = BOX_GRID
    case = rk.Case(n, (2, 2, 1), "periodic")
    Pr = sr.Problem(sc.faces(n, True), *sc.BC_SETS["periodic"], 0.002, "superbee")
    V = solenoidal(Pr)
    phi0 = 0.5 + 0.5 * sc.phi_field(n, "random") * sc.phi_field(n, "step")
    adv, dif = sr.cfl(Pr, V, 1.0)
    dt = 1.0 / (adv + dif)
    blocks = {"V": [rk.scatter_faces(case, V[a], a) for a in range(3)], "phi": rk.scatter_cells(case, phi0)}
    res = inproc.run_threads(case.size, _mass_worker, case, blocks, dt, 10)
    for r in range(case.size):
        assert res[r][0] == res[0][0], r                    # the statistics are the same bits on every rank
    states = [rk.gather_cells(case, [res[r][1][a] for r in range(case.size)]) for a in range(11)]
    vol = sr.volumes(Pr)
    depth = 0
    for r in range(case.size):
        ncell = int(np.prod(case.lo_len(r)[1]))
        nb = min(1024, -(-ncell // 256))
        depth = max(depth, -(-ncell // (256 * nb)) + 6 + 2 + nb + 3)
    depth += case.size
    m0, m1 = res[0][0][0][2], res[0][0][1][2]
    allowed = depth * sr.U * float((np.abs(phi0) * vol).sum())
    for before in states[:-1]:
        _, B = sr.step(Pr, before, V, dt, 5, None, np.longdouble, bounds=True)
        allowed += float((np.asarray(B, dtype=np.float64) * vol).sum())
    allowed += depth * sr.U * float((np.abs(states[-1]) * vol).sum())
    print(f"mass {m0!r} -> {m1!r}: moved {abs(m1 - m0):.3e}, allowed {allowed:.3e}")
    assert abs(m1 - m0) <= allowed * (1 + 2.0 ** -10)
    assert float(np.abs(states[-1] - phi0).max()) > 1e-2


def _box_worker(R, case, blocks, dt):
    import torch
    from fluca_amd.scalar import Scalar
    from tests.test_gpu_config5 import _handle
    P, d, s = _handle(R, case)
    out = {}
    with torch.cuda.stream(s):
        dev = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64).ravel(), device="cuda")
        S = Scalar(P, case.kinds, case.vals)
        S.set_velocity(*[dev(blocks["V"][a][R.rank]) for a in range(3)])
        out["cfl"] = S.cfl(dt)[0]
        for limiter in sr.BOUNDED + ("quick",):
            S.set_limiter(limiter)
            phid = dev(blocks["phi"][R.rank])
            lo, hi = 0.0, 1.0
            for _ in range(8):
                S.step(phid, dt, 5)
                mn, mx, _ = S.stats(phid)
                lo, hi = min(lo, mn), max(hi, mx)
            out[limiter] = (lo, hi)
        S.close()
    P.close()
    return out


@pytest.mark.parametrize("sign", [1.0, -1.0], ids=["plus", "minus"])
@pytest.mark.parametrize("axis", [0, 1, 2], ids=["x", "y", "z"])
def test_box_profile_stays_bounded_across_a_rank_face(axis, sign):
    """the set-up of tests/test_gpu_scalar_step.py::test_box_profile_stays_bounded on 2 x 1 x 1 ranks: along x the profile's edges cross the rank face
    and the periodic seam between the two ranks during the eight steps"""
    from tests.test_gpu_scalar_step import BOX_GRID
    n = BOX_GRID
    case = rk.Case(n, (2, 1, 1), "periodic")
    Pr = sc.problem(n, True, "periodic")
    V = [np.zeros(s) for s in Pr.shapes()[1]]
    V[axis][...] = sign
    dt = float(Pr.widths(axis)[0]) / 1.0
    idx = np.arange(n[axis])
    prof = ((idx >= n[axis] // 4) & (idx < (3 * n[axis]) // 4)).astype(np.float64)
    shp = [1, 1, 1]
    shp[2 - axis] = n[axis]
    phi0 = np.ascontiguousarray(np.broadcast_to(prof.reshape(shp), Pr.shapes()[0]))
    blocks = {"V": [rk.scatter_faces(case, V[a], a) for a in range(3)], "phi": rk.scatter_cells(case, phi0)}
    res = inproc.run_threads(case.size, _box_worker, case, blocks, dt)
    assert res[0] == res[1]
    assert res[0]["cfl"] == pytest.approx(1.0, rel=1e-12)
    for limiter in sr.BOUNDED + ("quick",):
        lo, hi = res[0][limiter]
        if limiter == "quick":
            assert lo < -0.1 and hi > 1.1, (limiter, lo, hi)
        else:
            assert lo >= -4 * ULP1 and hi <= 1 + 4 * ULP1, (limiter, lo, hi - 1)
