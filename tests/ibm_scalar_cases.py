"""The grids, marker sets and data of tests/test_ibm_scalar_host.py and tests/test_gpu_ibm_scalar*.py (no GPU).

Grid 24 x 20 x 16 (20 is no multiple of the 8-cell tile), walls in x and y, periodic in z; uniform (h = 1/16) or with x stretched towards its walls.
The marker set, 435 markers (no multiple of 4), in groups:

    sphere   150  radius 4 h about the middle of the box, spacing about 1.15 h: at least 2 cells from every wall
    knot     260  within +- 0.4 cells of one point inside a tile: a bin of more than 256 markers, two LDS chunks of k_ibm_spread
    seam      10  within half a cell of z = 0: supports that wrap through the periodic seam
    wall      10  within 0.3 h of the low x wall, within h of the high y wall: supports cut by a wall
    lattice    5  exactly on cell centres and faces

dV is the cell volume times U(0.5, 1.5) divided by the group's crowding (260 for the knot, 10 for seam and wall), so that one pass moves phi by
about the defect and five passes stay of order one.  Body ids interleave three bodies (l mod 3)."""
import numpy as np

from tests import ibm_regimes as R

N = (24, 20, 16)
BC = R.ZPER
PERIODIC = [False, False, True]
H = 1.0 / 16
BOX = [(0.0, 1.5), (0.0, 1.25), (0.0, 1.0)]
GROUPS = (("sphere", 150, 1.0), ("knot", 260, 260.0), ("seam", 10, 10.0), ("wall", 10, 10.0), ("lattice", 5, 1.0))
VALUES = np.array([1.0, -0.5, 2.0])
NPASSES = (1, 2, 5)


def grid(uniform):
    xf = R.uniform(N, BOX)
    if not uniform:
        xf[0] = R.stretched(N[0], *BOX[0], 1.3)
    return xf


def group_slices():
    out, at = {}, 0
    for name, count, _ in GROUPS:
        out[name] = slice(at, at + count)
        at += count
    return out


def markers(groups=None):
    """[X, Y, Z] of the groups named (default: all), in the order of GROUPS"""
    rng = np.random.default_rng(71)
    at = lambda d, s: BOX[d][0] + (np.asarray(s, dtype=np.float64) + 0.5) * H
    parts = {}
    parts["sphere"] = R.fib_sphere(150, (0.75, 0.625, 0.5), 4 * H)
    parts["knot"] = np.stack([at(d, c + rng.uniform(-0.4, 0.4, 260)) for d, c in enumerate((12.3, 11.6, 3.4))])
    seam = np.stack([at(0, rng.uniform(4.0, 19.0, 10)), at(1, rng.uniform(4.0, 15.0, 10)), rng.uniform(-0.5, 0.5, 10) * H])
    seam[2] = np.mod(seam[2], 1.0)
    parts["seam"] = seam
    wall = np.stack([at(0, rng.uniform(4.0, 19.0, 10)), at(1, rng.uniform(4.0, 15.0, 10)), at(2, rng.uniform(0.0, 15.0, 10))])
    wall[0, :5] = rng.uniform(0.0, 0.3, 5) * H                    # low x wall (inside the first cell of the stretched axis too)
    wall[1, 5:] = BOX[1][1] - rng.uniform(0.0, 1.0, 5) * H        # high y wall
    parts["wall"] = wall
    parts["lattice"] = np.stack([at(0, [5.0, 7.5, 8.0, 16.0, 15.5]), at(1, [8.0, 7.5, 4.0, 12.5, 9.0]), at(2, [7.5, 8.0, 0.0, 11.0, 3.5])])
    names = [g[0] for g in GROUPS] if groups is None else list(groups)
    X = np.concatenate([parts[k] for k in names], axis=1)
    return [np.ascontiguousarray(a, dtype=np.float64) for a in X]


def data(groups=None, seed=72):
    """dV, per-marker target T, body ids, phi0 of the markers of the groups named (the values of a group do not depend on which others are named)"""
    names = [g[0] for g in GROUPS] if groups is None else list(groups)
    ncell = N[0] * N[1] * N[2]
    rng = np.random.default_rng(seed)
    phi0 = rng.standard_normal(ncell)
    dV, T = {}, {}
    for name, count, crowd in GROUPS:
        dV[name] = rng.uniform(0.5, 1.5, count) * H ** 3 / crowd
        T[name] = rng.standard_normal(count)
    dV, T = np.concatenate([dV[k] for k in names]), np.concatenate([T[k] for k in names])
    body = (np.arange(T.size) % 3).astype(np.int32)
    return dict(dV=dV, T=T, body=body, phi0=phi0, Tbody=VALUES[body])


INNER = ("sphere", "knot", "seam")        # at least two cells from the walls in x and y: the whole support is inside or wraps


def contraction_set():
    """a sphere of radius 4 h with 200 markers (spacing about h), dV = h^3, T = 1, phi = 0"""
    X = [np.ascontiguousarray(a) for a in R.fib_sphere(200, (0.75, 0.625, 0.5), 4 * H)]
    return X, np.full(200, H ** 3), np.ones(200), np.zeros(N[0] * N[1] * N[2])


def conservation(xf, phi0, phi1, Q, dV):
    """sum_c (phi1 - phi0)_c vol_c, sum_l Q_l dV_l, and the margin: 1e-12 (the relative tolerance of the invariants of tests/test_gpu_ibm.py) of
    sum_c (|phi0| + |phi1|)_c vol_c + sum_l |Q_l| dV_l -- the differences and both sums round at u of those magnitudes"""
    vol = np.einsum("k,j,i->kji", *[np.diff(xf[a]) for a in (2, 1, 0)]).ravel()
    phi0, phi1, Q, dV = [np.asarray(a, dtype=np.float64).ravel() for a in (phi0, phi1, Q, dV)]
    lhs, rhs = float(((phi1 - phi0) * vol).sum()), float((Q * dV).sum())
    return lhs, rhs, 1e-12 * float(((np.abs(phi0) + np.abs(phi1)) * vol).sum() + (np.abs(Q) * dV).sum())
