"""fl_scalar_step on the GPU: against the rks2 step of tests/scalar_reference.py, and the properties a user relies on -- sum phi vol is conserved,
the bounded limiters keep a box profile inside [0, 1] at step CFL 1.

Every bound is derived (scalar_reference.step, bounds=True): the rounding bound of each stage's R, five roundings on the three terms of the stage
update, and what the earlier stages' error can have grown to -- carried through the sup-norm sensitivity A of R to its argument.  A step is
compared with the reference started from the GPU's own state before that step, so the bound is that of ONE step."""
import numpy as np
import pytest

from tests import scalar_cases as sc
from tests import scalar_reference as sr

pytestmark = pytest.mark.gpu

BOX_GRID = (16, 12, 20)
ULP1 = 2.0 ** -52


def _dev(a):
    from tests.gpu_common import dev
    return dev(np.ascontiguousarray(a).reshape(-1))


def _host(t, shape):
    from tests.gpu_common import host
    return host(t).reshape(shape).copy()


@pytest.mark.parametrize("n,uniform,bcname,limiters", [((7, 5, 6), False, "channel", ("superbee", "barthjesperson")), ((66, 9, 5), True, "periodic", ("vanleer", "vanalbada")),
                                                       ((4, 4, 4), False, "dirichlet", ("koren", "minmod")), ((7, 5, 6), True, "neumann", ("venkatakrishnan", "mc"))],
                         ids=["7x5x6-channel", "66x9x5-periodic", "4x4x4-dirichlet", "7x5x6-neumann"])
def test_three_steps_against_rks2(n, uniform, bcname, limiters):
    """s = 2, 3 and 5 in place by one handle; between them a second handle with another limiter, diffusivity and boundary values steps the SAME
    arrays: what a handle did before leaves no trace in what it does next."""
    from fluca_amd.scalar import Scalar
    Pz, S1 = sc.make_handles(n, uniform, bcname, limiter=limiters[0], gamma=0.0125)
    kinds, vals = sc.BC_SETS[bcname]
    vals2 = tuple(0.5 - v for v in vals)
    S2 = Scalar(Pz, kinds, vals2, limiter=limiters[1], gamma=0.004)
    P1 = sr.Problem(sc.faces(n, uniform), kinds, vals, 0.0125, limiters[0])
    P2 = sr.Problem(sc.faces(n, uniform), kinds, vals2, 0.004, limiters[1])
    V = sc.velocity(n, bcname)
    Vd = [_dev(v) for v in V]
    S1.set_velocity(*Vd)
    S2.set_velocity(*Vd)
    q = sc.source(n)
    qd = _dev(q)
    phi0 = sc.phi_field(n, "random") * 0.5 + sc.phi_field(n, "step")
    phid = _dev(phi0)
    adv, dif = sr.cfl(P1, V, 1.0)
    dt = 0.5 / (adv + dif)
    assert np.allclose(S1.cfl(dt), (adv * dt, dif * dt), rtol=1e-12)
    worst = 0.0
    for who, s, src in [(1, 2, None), (2, 3, q), (1, 3, q), (2, 5, None), (1, 5, q)]:
        before = _host(phid, phi0.shape)
        S, Pr = (S1, P1) if who == 1 else (S2, P2)
        S.step(phid, dt, s, None if src is None else qd)
        got = _host(phid, phi0.shape)
        want, B = sr.step(Pr, before, V, dt, s, src, np.longdouble, bounds=True)
        err = np.abs(got.astype(np.longdouble) - want).astype(np.float64)
        tol = np.asarray(B, dtype=np.float64) * (1 + 2.0 ** -10)
        worst = max(worst, float((err / tol).max()))
        assert (err <= tol).all(), (who, s, float(err.max()), float((err / tol).max()))
        assert float(np.abs(got - before).max()) > 1e-3          # (the step did something)
    print(f"step {n} {bcname}: largest error / bound = {worst:.3f}")
    S1.close()
    S2.close()
    Pz.close()


def solenoidal(Pr, seed=3):
    """the discrete curl of a seeded edge potential on a periodic grid: the discrete divergence of the face velocities is 0 up to rounding"""
    nx, ny, nz = Pr.n
    rng = np.random.default_rng(seed)
    Ax, Ay, Az = (rng.uniform(-0.05, 0.05, (nz, ny, nx)) for _ in range(3))
    hx, hy, hz = (Pr.widths(d) for d in range(3))
    ddx = lambda a: (np.roll(a, -1, 2) - a) / hx[None, None, :]
    ddy = lambda a: (np.roll(a, -1, 1) - a) / hy[None, :, None]
    ddz = lambda a: (np.roll(a, -1, 0) - a) / hz[:, None, None]
    V = (ddy(Az) - ddz(Ay), ddz(Ax) - ddx(Az), ddx(Ay) - ddy(Ax))
    div = ddx(V[0]) + ddy(V[1]) + ddz(V[2])
    assert np.abs(div).max() <= 64 * sr.U * max(np.abs(v).max() for v in V) / min(hx.min(), hy.min(), hz.min())
    return V


def test_mass_is_conserved():
    """10 steps, s = 5, in a solenoidal V on the periodic box: sum phi vol of fl_scalar_stats moves by no more than rounding -- per step the volume
    sum of the step's bound (the exact step conserves the sum: the fluxes telescope), and the two sums' own rounding (test_gpu_scalar.py)."""
    n = BOX_GRID
    Pz, S = sc.make_handles(n, True, "periodic", limiter="superbee", gamma=0.002)
    Pr = sr.Problem(sc.faces(n, True), *sc.BC_SETS["periodic"], 0.002, "superbee")
    V = solenoidal(Pr)
    S.set_velocity(*[_dev(v) for v in V])
    phi0 = 0.5 + 0.5 * sc.phi_field(n, "random") * sc.phi_field(n, "step")
    phid = _dev(phi0)
    adv, dif = sr.cfl(Pr, V, 1.0)
    dt = 1.0 / (adv + dif)
    vol = sr.volumes(Pr)
    ncell = phi0.size
    nb = min(1024, -(-ncell // 256))
    depth = -(-ncell // (256 * nb)) + 6 + 2 + nb + 3
    m0 = S.stats(phid)[2]
    allowed = depth * sr.U * float((np.abs(phi0) * vol).sum())
    for it in range(10):
        before = _host(phid, phi0.shape)
        S.step(phid, dt, 5)
        _, B = sr.step(Pr, before, V, dt, 5, None, np.longdouble, bounds=True)
        allowed += float((np.asarray(B, dtype=np.float64) * vol).sum())
    after = _host(phid, phi0.shape)
    m1 = S.stats(phid)[2]
    allowed += depth * sr.U * float((np.abs(after) * vol).sum())
    print(f"mass {m0!r} -> {m1!r}: moved {abs(m1 - m0):.3e}, allowed {allowed:.3e}")
    assert abs(m1 - m0) <= allowed * (1 + 2.0 ** -10)
    assert float(np.abs(after - phi0).max()) > 1e-2
    S.close()
    Pz.close()


@pytest.mark.parametrize("sign", [1.0, -1.0], ids=["plus", "minus"])
@pytest.mark.parametrize("axis", [0, 1, 2], ids=["x", "y", "z"])
def test_box_profile_stays_bounded(axis, sign):
    """uniform flow along one axis of the periodic box, a box profile, step CFL 1 (stage CFL 1/4), s = 5, eight steps: min and max of
    fl_scalar_stats stay within [0, 1] + 4 ulp of 1 for the nine bounded limiters and leave it for quick"""
    n = BOX_GRID
    Pz, S = sc.make_handles(n, True, "periodic")
    Pr = sc.problem(n, True, "periodic")
    shapes = Pr.shapes()[1]
    V = [np.zeros(s) for s in shapes]
    V[axis][...] = sign
    S.set_velocity(*[_dev(v) for v in V])
    h = float(Pr.widths(axis)[0])
    dt = h / 1.0
    idx = np.arange(n[axis])
    prof = ((idx >= n[axis] // 4) & (idx < (3 * n[axis]) // 4)).astype(np.float64)
    shp = [1, 1, 1]
    shp[2 - axis] = n[axis]
    phi0 = np.broadcast_to(prof.reshape(shp), Pr.shapes()[0])
    assert S.cfl(dt)[0] == pytest.approx(1.0, rel=1e-12)
    for limiter in sr.BOUNDED + ("quick",):
        S.set_limiter(limiter)
        phid = _dev(phi0)
        lo, hi = 0.0, 1.0
        for _ in range(8):
            S.step(phid, dt, 5)
            mn, mx, _ = S.stats(phid)
            lo, hi = min(lo, mn), max(hi, mx)
        if limiter == "quick":
            assert lo < -0.1 and hi > 1.1, (limiter, lo, hi)
        else:
            assert lo >= -4 * ULP1 and hi <= 1 + 4 * ULP1, (limiter, lo, hi - 1)
    S.close()
    Pz.close()
