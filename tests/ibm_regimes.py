"""Marker sets that take the immersed-boundary kernels (fluca_amd/csrc/fl_ibm.hip) out of the toy regime, named as tests/launch_regimes.py names
the grids of the other kernels: bins of more than 256 and 512 markers (k_ibm_spread's chunk loop, k_ibm_sort_bins' strided loop), more than 4096
tiles and exactly 4096 (k_ibm_scan's carry), marker counts that are no multiple of 4 (k_ibm_interp's partial last block), markers exactly on
cell centres and faces, coincident markers, markers beyond walls and beyond the ends of a periodic axis.

Every set is generated from seeds; `reach` holds, per delta function (0 Peskin-4, 1 Roma-3), the regime fields it must reach on its first boundary
types -- tests/test_ibm_regimes.py recomputes them with tests/ibm_reference.bins, so that an edit of a set cannot silently leave its regime.
tests/test_gpu_ibm_regimes.py runs the kernels on all of them."""
import numpy as np

from oracle import fluca_oracle as fo

V, O, PER = fo.BC_VELOCITY, fo.BC_PRESSURE_OUTLET, fo.BC_PERIODIC
WALLS = [V] * 6
XZPER = [PER, PER, V, V, PER, PER]
YZPER = [V, V, PER, PER, PER, PER]
ZPER = [V, V, V, V, PER, PER]
BCNAME = {tuple(WALLS): "walls", tuple(XZPER): "xzper", tuple(YZPER): "yzper", tuple(ZPER): "zper", (V, O, V, V, PER, PER): "channel"}


def stretched(n, lo, hi, beta):
    s = np.linspace(0.0, 1.0, n + 1)
    return lo + (hi - lo) * (np.tanh(beta * (2 * s - 1)) / np.tanh(beta) + 1) / 2


def fib_sphere(L, centre, R):
    i = np.arange(L) + 0.5
    ph = np.arccos(1 - 2 * i / L)
    th = np.pi * (1 + 5 ** 0.5) * i
    return np.stack([centre[0] + R * np.cos(th) * np.sin(ph), centre[1] + R * np.sin(th) * np.sin(ph), centre[2] + R * np.cos(ph)])


class IbmRegime:
    """n, face coordinates xf, the boundary types it is run with (bcs), markers() -> [X, Y, Z], and reach = {kind: fields}"""

    def __init__(self, name, n, xf, bcs, markers, reach, interior=None, ranks=(1, 1, 1)):
        self.name, self.n, self.xf, self.bcs, self._markers, self.reach, self.ranks = name, tuple(n), xf, bcs, markers, reach, ranks
        self._interior = interior

    def markers(self):
        return [np.ascontiguousarray(a, dtype=np.float64) for a in self._markers(self)]

    def interior(self):
        """the markers whose whole support lies inside the domain or wraps, on every one of bcs (None: no invariants on this set)"""
        return None if self._interior is None else self._interior(self)

    def at(self, d, s):
        """position of the cell-centre index s on the uniform axis d"""
        xf = self.xf[d]
        return xf[0] + (np.asarray(s, dtype=np.float64) + 0.5) * ((xf[-1] - xf[0]) / self.n[d])

    @staticmethod
    def periodic(bc):
        return [bc[0] == PER, bc[2] == PER, bc[4] == PER]


def uniform(n, box):
    return [np.linspace(box[d][0], box[d][1], n[d] + 1) for d in range(3)]


# ---------------------------------------------------------------------------------------------------------------------------- dense_shell

def _dense_shell(r):
    h = 1.0 / 200
    big = fib_sphere(20107, [r.at(d, c) for d, c in enumerate((132.0, 100.0, 70.0))], 20 * h)        # 4 markers per h^2: the usual h / 2 mesh
    small = fib_sphere(2001, [r.at(d, c) for d, c in enumerate((40.3, 30.2, 12.1))], 9.7 * h)
    knot = np.repeat(np.array([[r.at(0, 200.37)], [r.at(1, 150.5)], [r.at(2, 120.25)]]), 701, axis=1)  # 701 coincident markers
    return list(np.concatenate([big, small, knot], axis=1))


DENSE_SHELL = IbmRegime("dense_shell", (264, 200, 136), uniform((264, 200, 136), [(0.0, 1.32), (0.0, 1.0), (0.0, 0.68)]), [WALLS, XZPER], _dense_shell,
                        {0: dict(max_bin=701, min_over_256=100, min_over_512=40, scan_rounds=[0, 1, 2, 3], ntiles=14025, L_mod_4=1),
                         1: dict(max_bin=701, min_over_256=80, min_over_512=4, scan_rounds=[0, 1, 2, 3], ntiles=14025, L_mod_4=1)},
                        interior=lambda r: np.arange(22809))


# ---------------------------------------------------------------------------------------------------------------------------- scan_exact / scan_ragged

def _clusters(r, cells, count, seed, half=2.4):
    """count markers uniformly within +- half cells of each of the cell-index points given"""
    rng = np.random.default_rng(seed)
    parts = [np.stack([r.at(d, c[d] + rng.uniform(-half, half, count)) for d in range(3)]) for c in cells]
    return np.concatenate(parts, axis=1)


def _scan_exact(r):
    cl = _clusters(r, [(3.5, 3.5, 3.5), (123.5, 123.5, 123.5), (64.0, 3.5, 127.0 - 3.5)], 90, 11)
    sp = fib_sphere(301, [r.at(d, 63.7) for d in range(3)], 0.11)
    return list(np.concatenate([cl, sp], axis=1))


SCAN_EXACT = IbmRegime("scan_exact", (128, 128, 128), uniform((128, 128, 128), [(0.0, 1.0)] * 3), [WALLS], _scan_exact,
                       {k: dict(scan_rounds=[0], ntiles=4096, first_tile=0, last_tile=4095, L_mod_4=3) for k in (0, 1)},
                       interior=lambda r: np.arange(571))


def _scan_ragged(r):
    # 17 tiles per axis, the last one partial on each (131 = 16*8 + 3, 133 = 16*8 + 5, 135 = 16*8 + 7).  Tile t = (tz * 17 + ty) * 17 + tx:
    # tile 0, tiles 4095 | 4096 = (tz 14, ty 2, tx 15 | 16), the last tile 4912, and one in the middle
    cl = _clusters(r, [(3.5, 3.5, 3.5), (127.8, 19.5, 115.5), (129.3, 130.6, 132.2), (60.0, 70.0, 60.0)], 80, 12, half=1.2)
    rng = np.random.default_rng(13)
    cloud = np.stack([r.at(d, rng.uniform(2.0, r.n[d] - 3.0, 503)) for d in range(3)])
    return list(np.concatenate([cl, cloud], axis=1))


SCAN_RAGGED = IbmRegime("scan_ragged", (131, 133, 135), uniform((131, 133, 135), [(0.0, 1.31), (0.0, 1.33), (0.0, 1.35)]), [WALLS, XZPER], _scan_ragged,
                        {k: dict(scan_rounds=[0, 1], ntiles=4913, first_tile=0, last_tile=4912, L_mod_4=3, tiles_hit=[0, 4095, 4096, 4912]) for k in (0, 1)},
                        interior=lambda r: np.concatenate([np.arange(80), np.arange(240, 823)]))      # two clusters hug the high walls


# ---------------------------------------------------------------------------------------------------------------------------- dense_stretched

def _stretched_xf(n):
    box = [(0.0, 1.0), (0.0, 2.0), (0.0, 1.5)]
    return [stretched(n[0], *box[0], 1.4), stretched(n[1], *box[1], 1.7), np.linspace(*box[2], n[2] + 1)]


def _dense_stretched(r):
    sp = fib_sphere(400, (0.5, 1.0, 0.75), 0.35)
    rng = np.random.default_rng(14)
    # 303 markers within the first three cells of the refined x wall (through the mirror-image ghost centre) and the first tile in y
    xw = rng.uniform(r.xf[0][0], r.xf[0][3], 303)
    yw = rng.uniform(r.xf[1][0], r.xf[1][5], 303)
    zw = rng.uniform(0.70, 0.80, 303)
    return [np.concatenate([sp[0], xw]), np.concatenate([sp[1], yw]), np.concatenate([sp[2], zw])]


DENSE_STRETCHED = IbmRegime("dense_stretched", (48, 40, 24), _stretched_xf((48, 40, 24)), [ZPER], _dense_stretched,
                            {k: dict(min_max_bin=303, min_over_256=1, L_mod_4=3) for k in (0, 1)}, interior=lambda r: np.arange(400))


# ---------------------------------------------------------------------------------------------------------------------------- lattice

def _lattice(r):
    """every combination of {cell centres, faces} x {at the low end, one in, across a tile edge, at the high end} per axis, each one twice, and one
    more: x uniform, y uniform, z stretched (positions exactly ON the stored faces / centres)"""
    pts = []
    for d in range(3):
        n, xf = r.n[d], r.xf[d]
        cen, fac = [0, 1, 7, 8, n - 1], [0, 1, 8, n]
        if d < 2:
            pts.append(np.concatenate([r.at(d, np.array(cen, dtype=float)), r.at(d, np.array(fac, dtype=float) - 0.5)]))
        else:
            pts.append(np.concatenate([(xf[:-1] + xf[1:])[cen] / 2.0, xf[fac]]))
    Z, Y, X = np.meshgrid(pts[2], pts[1], pts[0], indexing="ij")
    one = np.stack([X.ravel(), Y.ravel(), Z.ravel()])
    return list(np.concatenate([one, one, one[:, 364:365]], axis=1))


_LN = (24, 20, 16)
LATTICE = IbmRegime("lattice", _LN, [np.linspace(0.0, 1.5, 25), np.linspace(0.0, 1.25, 21), stretched(16, 0.0, 1.0, 1.3)], [XZPER, YZPER, WALLS], _lattice,
                    {k: dict(L_mod_4=3) for k in (0, 1)})


# ---------------------------------------------------------------------------------------------------------------------------- stray

_SN, _SBOX = (32, 16, 64), [(0.0, 2.0), (0.0, 1.0), (0.0, 4.0)]        # h = 1/16 on every axis, box lengths powers of two: X + period is exact


def _snap(x):
    return np.round(np.asarray(x, dtype=np.float64) * 2.0 ** 20) / 2.0 ** 20


def stray_parts(r):
    """the groups of the stray set, in order -> {name: (3, count) positions}.  Positions are multiples of 2^-20."""
    rng = np.random.default_rng(15)
    mid = lambda count: np.stack([_snap(r.at(d, rng.uniform(5.0, r.n[d] - 6.0, count))) for d in range(3)])
    parts = {"inside": mid(39)}
    # supports wholly beyond each of the six walls, by 3 and by 40 cells
    wall = mid(12)
    for j, (d, side, by) in enumerate((d, side, by) for d in range(3) for side in (0, 1) for by in (3.0, 40.0)):
        wall[d, j] = r.at(d, -0.5 - by - 0.3) if side == 0 else r.at(d, r.n[d] - 0.5 + by + 0.3)
    parts["beyond_walls"] = _snap(wall)
    # beyond either end of the axes that XZPER makes periodic: within one period, between one and two, 5.3 periods
    for key, periods in (("one_period", 0.37), ("two_periods", 1.62), ("far", 5.3)):
        p = mid(4)
        for j, (d, side) in enumerate((d, side) for d in (0, 2) for side in (0, 1)):
            span = r.xf[d][-1] - r.xf[d][0]
            p[d, j] = r.xf[d][0] - periods * span if side == 0 else r.xf[d][-1] + periods * span
        parts[key] = _snap(p)
    # the one_period markers shifted back into the box by exactly one period
    back = parts["one_period"].copy()
    for j, (d, side) in enumerate((d, side) for d in (0, 2) for side in (0, 1)):
        back[d, j] += (r.xf[d][-1] - r.xf[d][0]) * (1 if side == 0 else -1)
    parts["one_period_back"] = back
    return parts


def stray_groups(r):
    """{name: indices into markers()}"""
    out, at = {}, 0
    for k, v in stray_parts(r).items():
        out[k] = np.arange(at, at + v.shape[1])
        at += v.shape[1]
    return out


def _stray(r):
    return list(np.concatenate(list(stray_parts(r).values()), axis=1))


STRAY = IbmRegime("stray", _SN, uniform(_SN, _SBOX), [WALLS, XZPER], _stray, {k: dict(L=67, L_mod_4=3) for k in (0, 1)})
STRAY_1 = IbmRegime("stray_1", _SN, uniform(_SN, _SBOX), [XZPER, WALLS], lambda r: [a[55:56] for a in _stray(STRAY)], {k: dict(L=1, L_mod_4=1) for k in (0, 1)})
STRAY_63 = IbmRegime("stray_63", _SN, uniform(_SN, _SBOX), [XZPER, WALLS], lambda r: [a[4:67] for a in _stray(STRAY)], {k: dict(L=63, L_mod_4=3) for k in (0, 1)})


# ---------------------------------------------------------------------------------------------------------------------------- dense_face (two ranks)

def _dense_face(r):
    # the face between the two z ranks (cell 16 of 32) cuts through a cube of 620 markers; 131 more on the periodic seam, the ranks' other face
    a = _clusters(r, [(12.3, 10.2, 16.1)], 620, 16, half=2.5)
    b = _clusters(r, [(12.6, 9.7, -0.4)], 131, 17, half=2.0)
    b[2] = (b[2] - r.xf[2][0]) % (r.xf[2][-1] - r.xf[2][0]) + r.xf[2][0]
    return list(np.concatenate([a, b], axis=1))


_FN = (24, 20, 32)
DENSE_FACE = IbmRegime("dense_face", _FN, uniform(_FN, [(0.0, 1.5), (0.0, 1.25), (0.0, 2.0)]), [[V, O, V, V, PER, PER]], _dense_face,
                       {k: dict(min_block_bin=257, L_mod_4=3) for k in (0, 1)}, interior=lambda r: np.arange(751), ranks=(1, 1, 2))


REGIMES = [DENSE_SHELL, SCAN_EXACT, SCAN_RAGGED, DENSE_STRETCHED, LATTICE, STRAY, STRAY_1, STRAY_63, DENSE_FACE]
BY_NAME = {r.name: r for r in REGIMES}
SINGLE = [r for r in REGIMES if r.ranks == (1, 1, 1)]


def fields(r, kind, bc=None, block=None):
    from tests import ibm_reference as ref
    bc = r.bcs[0] if bc is None else bc
    return ref.regime_fields(r.n, kind, r.markers(), r.periodic(bc), r.xf, block=block)


def check_reach(r, kind, got):
    """assert that the regime fields `got` (ibm_reference.regime_fields) satisfy the entry of r"""
    want = r.reach[kind]
    L = r.markers()[0].size
    for key, val in want.items():
        if key == "L":
            assert L == val, (r.name, key, L)
        elif key == "min_over_256":
            assert got["bins_over_256"] >= val, (r.name, key, got)
        elif key == "min_over_512":
            assert got["bins_over_512"] >= val, (r.name, key, got)
        elif key in ("min_max_bin", "min_block_bin"):
            assert got["max_bin"] >= val, (r.name, key, got)
        elif key == "tiles_hit":
            assert all(got["counts"][t] > 0 for t in val), (r.name, key, [int(got["counts"][t]) for t in val])
        else:
            assert got[key] == val, (r.name, key, got[key], val)
