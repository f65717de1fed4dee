"""What the tests of the implicit scalar diffusion on several ranks share (tests/test_scalar_implicit_ranks_host.py, tests/test_gpu_scalar_implicit_ranks*.py):
the cases, the inputs of a case, and the wire of include/fluca_hip_implicit_ranks.h counted from geometry -- numpy only, no GPU, no library.

The 7-point star reaches one cell across a rank face, so ONE exchange of the implicit path ships one plane of doubles across every boundary of a
rank's block with a neighbouring rank: the messages of scalar_ranks.wire_phi, half its bytes.  Per call
    apply          1 exchange
    solve          k exchanges (k: the Chebyshev steps, info["steps"])
    IMEX theta = 1 the wire of fl_scalar_step(dt, s) on the handle (scalar_ranks.wire_step: the high faces of V once, two planes of phi per stage) + k exchanges
    IMEX theta < 1 that + 1 exchange (phi^n, for D(phi^n))
and no all-reduce anywhere."""
import functools

import numpy as np

from tests import scalar_cases as sc
from tests import scalar_implicit_reference as ir
from tests import scalar_ranks as rk
from tests import scalar_reference as sr

STAGES = 3
RTOL = 1e-6
MAXIT = 100000
S_APPLY, S_SOLVE = 5.0, 20.0          # S = c sum_d max omega_d: kappa = 1 + 2 S
COURANT, DIFFUSIVE = 0.4, 20.0        # fl_scalar_cfl's two numbers of the IMEX step
THETAS = (1.0, 0.5)
PLAN_BLOCK = (65, 64, 40)             # a rank's block of the case (65, 64, 80) on 1 x 1 x 2: fixed_seg set, 160 of the 256 blocks per XCD that are k_scalar_cheb's cap
CAP_BLOCK = (65, 64, 65)              # the smallest block of 65 x 64 cells a plane that DOES take cheb_plan's blocks per XCD at their cap (the plan of 512 x 512 x 256), and
                                      # sends some waves through their loop a second time: a rank's block of the case (65, 64, 130) on 1 x 1 x 2


def cases():
    """the smallest shapes that reach each way k_scalar_cheb_ring can go wrong"""
    out = []
    for ranks in [(2, 1, 1), (1, 2, 1), (1, 1, 2)]:                     # a split periodic axis of two-cell blocks: both planes from one peer, every cell a send layer
        out.append(rk.Case((4, 4, 4), ranks, "periodic"))
    for bcname in ("dirichlet", "periodic"):                             # a middle rank with two neighbours
        out.append(rk.Case((6, 5, 4), (3, 1, 1), bcname, uniform=False))
        out.append(rk.Case((4, 5, 6), (1, 1, 3), bcname, uniform=False))
    for bcname in sc.BC_SETS:
        for uniform in (True, False):                                    # a two-cell block between a rank face and a physical boundary
            out.append(rk.Case((7, 5, 6), (2, 1, 1), bcname, uniform=uniform, own=[(5, 2), (5,), (6,)]))
        out.append(rk.Case((7, 6, 5), (2, 2, 2), bcname, uniform=False))   # config 5's rank grid; channel splits its periodic z
    for ranks in [(2, 1, 1), (1, 2, 1), (1, 1, 2)]:                     # rows of three wave segments (two on a rank of 2 x 1 x 1: the x rank face at a ragged segment end)
        out.append(rk.Case((130, 6, 7), ranks, "channel", uniform=False))
    out.append(rk.Case((65, 64, 80), (1, 1, 2), "channel", uniform=False))   # each block PLAN_BLOCK
    out.append(rk.Case((65, 64, 130), (1, 1, 2), "channel", uniform=False))  # each block CAP_BLOCK
    return out


CHANNEL_222 = ((7, 6, 5), (2, 2, 2), "channel", False)


def case_key(case):
    """what the one-rank reference of a case depends on: the global grid, not the rank grid"""
    return (case.n, case.bcname, case.uniform)


def wire_exchange(case, rank):
    """(messages, bytes) a rank sends in ONE one-plane exchange"""
    nb = case.neighbours(rank)
    return sum(nb), sum(8 * rk.plane(case, rank, b // 2) for b in range(6) if nb[b])


def _times(k, w):
    return k * w[0], k * w[1]


def wire_apply(case, rank):
    """-> (exchanges, messages, bytes)"""
    return (1,) + wire_exchange(case, rank)


def wire_solve(case, rank, k):
    return (k,) + _times(k, wire_exchange(case, rank))


def wire_explicit_step(case, rank, s):
    """fl_scalar_step on the handle: one exchange of V's high faces, s of phi"""
    return (s + 1,) + rk.wire_step(case, rank, s)


def wire_imex(case, rank, s, k, theta):
    extra = k + (1 if theta < 1.0 else 0)
    ex, m, b = wire_explicit_step(case, rank, s)
    xm, xb = _times(extra, wire_exchange(case, rank))
    return ex + extra, m + xm, b + xb


@functools.lru_cache(maxsize=None)
def inputs(n, bcname, uniform):
    """the global fields and numbers of the five calls of a case: apply; solve to RTOL at S = 20; solve with maxit = 2; step_imex with theta = 1 and 1 / 2 at a
    Courant number of 0.4 and a diffusive number of 20"""
    Pr = sc.problem(n, uniform, bcname)
    rng = np.random.default_rng(20261021)
    shape = Pr.shapes()[0]
    V = sc.velocity(n, bcname)
    dt = COURANT / sr.cfl(Pr, V, 1.0)[0]
    gamma = DIFFUSIVE / sr.cfl(ir.with_gamma(Pr, 1.0), V, dt)[1]
    return dict(c_apply=ir.c_for_S(Pr, S_APPLY), c_solve=ir.c_for_S(Pr, S_SOLVE), phi=sc.phi_field(n, "random"), b=rng.uniform(-1, 1, shape), x0=rng.uniform(-1, 1, shape),
                V=V, dt=dt, gamma=gamma, q=sc.source(n), phi0=0.5 * sc.phi_field(n, "random") + sc.phi_field(n, "step"))


def scatter(case, I):
    """the blocks of every field of inputs(), per rank"""
    out = {k: rk.scatter_cells(case, I[k]) for k in ("phi", "b", "x0", "q", "phi0")}
    out["V"] = [rk.scatter_faces(case, I["V"][a], a) for a in range(3)]
    return out
