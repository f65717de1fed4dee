"""Grids, boundary sets and fields shared by the passive-scalar tests (tests/test_gpu_scalar*.py): seeded, built once per session."""
import functools

import numpy as np

from tests import scalar_reference as sr

D, N, P = sr.DIRICHLET, sr.NEUMANN, sr.PERIODIC
BOX = [(0.0, 1.0), (0.0, 1.0), (0.0, 0.5)]

# name -> (kinds, values); a Neumann value is the derivative along the +axis
BC_SETS = {
    "periodic": ((P,) * 6, (0.0,) * 6),
    "channel": ((D, N, N, N, P, P), (0.7, 0.0, 0.3, -0.2, 0.0, 0.0)),      # Dirichlet x-, Neumann 0 at x+, Neumann in y, periodic z
    "dirichlet": ((D,) * 6, (0.7, -0.4, 0.25, 1.5, -1.1, 0.6)),
    "neumann": ((N,) * 6, (0.9, -0.6, 0.35, 1.2, -0.8, 0.5)),
}

# The smallest grid that takes the launch plan of 512^3 (fldbg_scalar_plan: the blocks per XCD at their cap, every wave keeping one x segment)
# AND gives some waves a second trip through their loop, which no smaller grid does: 2 ragged x segments, 5120 row segments for 4096 waves.
REGIME_GRID = (65, 64, 40)


def poisson_bc(kinds):
    """the flow boundary types of a fl_poisson handle with the same periodic axes (the scalar's other kinds have no flow counterpart: walls)"""
    from oracle import fluca_oracle as fo
    return [fo.BC_PERIODIC if k == P else fo.BC_VELOCITY for k in kinds]


def faces(n, uniform):
    if uniform:
        return [BOX[d][0] + (BOX[d][1] - BOX[d][0]) * np.arange(n[d] + 1, dtype=np.float64) / n[d] for d in range(3)]
    from tests.gpu_common import stretched_faces
    return stretched_faces(n, BOX)


@functools.lru_cache(maxsize=None)
def problem(n, uniform, bcname):
    kinds, vals = BC_SETS[bcname]
    return sr.Problem(faces(n, uniform), kinds, vals)


@functools.lru_cache(maxsize=None)
def velocity(n, bcname, seed=20261019):
    """seeded, both signs, about a tenth of the faces exactly 0; the boundary faces get both signs too: inflow and outflow"""
    Pr = problem(n, True, bcname)
    rng = np.random.default_rng(seed)
    V = []
    for shp in Pr.shapes()[1]:
        v = rng.uniform(-1.0, 1.0, shp)
        v[rng.uniform(size=shp) < 0.1] = 0.0
        V.append(v)
    return tuple(V)


PHI_KINDS = ("random", "plateau", "step", "ramp", "alternating")


@functools.lru_cache(maxsize=None)
def phi_field(n, kind, seed=7):
    nx, ny, nz = n
    rng = np.random.default_rng(seed)
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    if kind == "random":
        return rng.uniform(-1.0, 1.0, (nz, ny, nx))
    if kind == "plateau":      # gradients exactly 0 on more than half the cells: the r = 1 guard fires
        a = rng.uniform(-1.0, 1.0, (nz, ny, nx))
        a[(i + j + k) % 7 < 5] = 0.375
        return a
    if kind == "step":
        return np.where(2 * i + 3 * j + 5 * k < (2 * nx + 3 * ny + 5 * nz) // 2, 1.0, 0.0)
    if kind == "ramp":
        return 0.25 + 0.125 * i - 0.0625 * j + 0.03125 * k
    if kind == "alternating":  # every cell an extremum along every axis: r < 0
        return (1.0 - 2.0 * ((i + j + k) % 2)) * (1.0 + 0.25 * rng.uniform(size=(nz, ny, nx)))
    raise ValueError(kind)


@functools.lru_cache(maxsize=None)
def source(n, seed=11):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, (n[2], n[1], n[0]))


def make_handles(n, uniform, bcname, **kw):
    """-> (Poisson, Scalar) on the grid of problem(n, uniform, bcname)"""
    from fluca_amd.poisson import Poisson
    from fluca_amd.scalar import Scalar
    kinds, vals = BC_SETS[bcname]
    Pz = Poisson(n, faces(n, uniform), poisson_bc(kinds), 1e-3)
    return Pz, Scalar(Pz, kinds, vals, **kw)


def rhs_slack(E):
    """the bound of scalar_reference.rhs in absolute terms: E U, a 2^-10 share for the second-order terms and the long-double reference's own
    rounding, and the smallest normal number for results that are exactly 0"""
    return np.asarray(E, dtype=np.float64) * sr.U * (1 + 2.0 ** -10) + np.finfo(np.float64).tiny
