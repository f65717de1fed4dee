"""The IBM paragraph of DESIGN.md once more, in numpy long double, independent of the oracle (oracle/fluca_oracle.c fo_ibm_*) and of the kernels
(fluca_amd/csrc/fl_ibm.hip): both of those were written by the same hand from the same text, and no reference implementation exists.

The spec:  a marker at X is mapped, axis by axis, to the continuous cell-centre index s -- (X - x0) / h - 1/2 on a uniform axis; on a stretched
one piecewise linear through the cell centres, beyond the first / last centre through its mirror image in the wall or the periodic image, and
linearly on beyond that.  The support starts at cell floor(s) - 1 (Peskin, 4 cells) or floor(s + 1/2) - 1 (Roma, 3 cells), the 1-D weights
are phi(s - i).  An index on a periodic axis is taken modulo the number of cells; a cell beyond a wall is dropped.  U = sum w u;
f_cell += F dV w / V_cell, V_cell = h^3 on a uniform grid and dx_i dy_j dz_k otherwise.

What counts as DATA here, not as arithmetic under test: the face coordinates, and the cell centres (x_i + x_{i+1}) / 2 with their two ghost
centres, formed in double as the grid stores them.  Everything from the marker position on is long double."""
import numpy as np

LD = np.longdouble
PESKIN4, ROMA3 = 0, 1
TB = 8           # tile edge of k_ibm_spread's bins


def phi(kind, r):
    r = np.abs(np.asarray(r, dtype=LD))
    out = np.zeros_like(r)
    one, half = LD(1), LD(1) / 2
    if kind == PESKIN4:
        a = r <= one
        out[a] = (3 - 2 * r[a] + np.sqrt(1 + 4 * r[a] - 4 * r[a] * r[a])) / 8
        b = ~a & (r <= 2)
        out[b] = (5 - 2 * r[b] - np.sqrt(np.maximum(-7 + 12 * r[b] - 4 * r[b] * r[b], 0))) / 8
    else:
        a = r <= half
        out[a] = (1 + np.sqrt(1 - 3 * r[a] * r[a])) / 3
        b = ~a & (r <= one + half)
        out[b] = (5 - 3 * r[b] - np.sqrt(np.maximum(1 - 3 * (1 - r[b]) * (1 - r[b]), 0))) / 6
    return out


def is_uniform(xf):
    xf = np.asarray(xf, dtype=np.float64)
    h = (xf[-1] - xf[0]) / (xf.size - 1)
    return bool(np.all(np.abs(np.diff(xf) - h) <= 1e-10 * h))


def centres(xf, periodic):
    """centres -1 .. n as the grid stores them (double)"""
    xf = np.asarray(xf, dtype=np.float64)
    xc = (xf[:-1] + xf[1:]) / 2.0
    if periodic:
        return np.concatenate([[xc[-1] - (xf[-1] - xf[0])], xc, [xc[0] + (xf[-1] - xf[0])]])
    return np.concatenate([[2.0 * xf[0] - xc[0]], xc, [2.0 * xf[-1] - xc[-1]]])


def index(xf, periodic, X):
    """continuous cell-centre index of the positions X along one axis"""
    xf = np.asarray(xf, dtype=np.float64)
    n = xf.size - 1
    X = np.asarray(X, dtype=np.float64).astype(LD)
    if is_uniform(xf):
        h = (LD(xf[-1]) - LD(xf[0])) / LD(n)
        return (X - LD(xf[0])) / h - LD(1) / 2
    ext = centres(xf, periodic).astype(LD)                       # ext[j] is centre j - 1
    j = np.clip(np.searchsorted(ext, X, side="right") - 1, 0, n)  # ext[j] <= X < ext[j + 1], clamped: linear extension beyond the ghosts
    return (j - 1).astype(LD) + (X - ext[j]) / (ext[j + 1] - ext[j])


def support_1d(kind, xf, periodic, X):
    """-> cells (L, S) int64, -1 where the cell lies beyond a wall; weights (L, S) long double"""
    n = np.asarray(xf).size - 1
    S = 4 if kind == PESKIN4 else 3
    s = index(xf, periodic, X)
    first = (np.floor(s) if kind == PESKIN4 else np.floor(s + LD(1) / 2)).astype(np.int64) - 1
    cells = first[:, None] + np.arange(S)[None, :]
    w = phi(kind, s[:, None] - cells.astype(LD))
    cells = cells % n if periodic else np.where((cells >= 0) & (cells < n), cells, -1)
    return cells, w


def _support(n, xf, periodic, kind, X):
    """flat cell index (L, S, S, S) (z slowest), validity mask, weight products"""
    (ci, wx), (cj, wy), (ck, wz) = [support_1d(kind, xf[d], periodic[d], X[d]) for d in range(3)]
    ok = (ck[:, :, None, None] >= 0) & (cj[:, None, :, None] >= 0) & (ci[:, None, None, :] >= 0)
    cell = (ck[:, :, None, None] * n[1] + cj[:, None, :, None]) * n[0] + ci[:, None, None, :]
    W = wz[:, :, None, None] * wy[:, None, :, None] * wx[:, None, None, :]
    return np.where(ok, cell, 0), ok, np.where(ok, W, LD(0))


def interp(n, xf, periodic, kind, X, u):
    """u (ncomp, ncell) -> U (ncomp, L) long double, A = sum |w| |u| and max |u| over the support (ncomp, L) double"""
    cell, ok, W = _support(n, xf, periodic, kind, X)
    u = np.asarray(u, dtype=np.float64).reshape(-1, n[0] * n[1] * n[2])
    L = cell.shape[0]
    U, A, M = np.zeros((u.shape[0], L), dtype=LD), np.zeros((u.shape[0], L)), np.zeros((u.shape[0], L))
    for c in range(u.shape[0]):
        uu = np.where(ok, u[c][cell], 0.0)
        U[c] = (W * uu.astype(LD)).reshape(L, -1).sum(axis=1)
        A[c] = (np.abs(W).astype(np.float64) * np.abs(uu)).reshape(L, -1).sum(axis=1)
        M[c] = np.abs(uu).reshape(L, -1).max(axis=1)
    return U, A, M


def cell_volumes(n, xf, cells):
    """volume of the flat cells: h^3 on a uniform grid, dx_i dy_j dz_k otherwise (long double)"""
    xf = [np.asarray(a, dtype=np.float64) for a in xf]
    if all(is_uniform(a) for a in xf):
        h = [(LD(a[-1]) - LD(a[0])) / LD(a.size - 1) for a in xf]
        return np.full(cells.shape, h[0] * h[1] * h[2], dtype=LD)
    dx = [np.diff(a.astype(LD)) for a in xf]
    i, j, k = cells % n[0], (cells // n[0]) % n[1], cells // (n[0] * n[1])
    return dx[0][i] * dx[1][j] * dx[2][k]


def spread(n, xf, periodic, kind, X, dV, F):
    """-> cells (sorted flat indices of the cells some marker reaches), add (ncomp, cells) long double = sum_l F_l dV_l w_l / V_cell,
    B (ncomp, cells) double = sum_l |F_l| dV_l / V_cell over the markers reaching the cell, m (cells) = how many markers reach it"""
    cell, ok, W = _support(n, xf, periodic, kind, X)
    F = np.asarray(F, dtype=np.float64).reshape(-1, cell.shape[0])
    dV = np.asarray(dV, dtype=np.float64)
    cells, inv = np.unique(cell[ok], return_inverse=True)
    vol = cell_volumes(n, xf, cells)
    lidx = np.broadcast_to(np.arange(cell.shape[0])[:, None, None, None], cell.shape)[ok]
    Wok = W[ok]
    add, B = np.zeros((F.shape[0], cells.size), dtype=LD), np.zeros((F.shape[0], cells.size))
    for c in range(F.shape[0]):
        FdV = F[c].astype(LD) * dV.astype(LD)
        np.add.at(add[c], inv, Wok * FdV[lidx] / vol[inv])
        B[c] = np.bincount(inv, weights=(np.abs(FdV[lidx]) / vol[inv]).astype(np.float64), minlength=cells.size)
    return cells, add, B, np.bincount(inv, minlength=cells.size)


def bins(n, kind, X, periodic, xf, block=None):
    """markers per 8 x 8 x 8 tile (flat, x fastest): a marker is in the bin of every tile that holds a cell of its support.
    block = (lo, length) per axis: the tiles of that block of a several-rank grid, over the support cells the block owns"""
    lo, ln = block if block is not None else ((0, 0, 0), n)
    nt = [(ln[d] + TB - 1) // TB for d in range(3)]
    L = np.asarray(X[0]).size
    tiles = []
    for d in range(3):
        cells, _ = support_1d(kind, xf[d], periodic[d], X[d])
        cells = np.where((cells >= lo[d]) & (cells < lo[d] + ln[d]), cells - lo[d], -1)
        t = np.where(cells >= 0, cells // TB, -1)
        t = np.sort(t, axis=1)
        t[:, 1:][t[:, 1:] == t[:, :-1]] = -1                       # the distinct tiles of the support, -1 elsewhere
        tiles.append(t)
    cnt = np.zeros(nt[0] * nt[1] * nt[2], dtype=np.int64)
    S = tiles[0].shape[1]
    for c in range(S):
        for b in range(S):
            for a in range(S):
                tx, ty, tz = tiles[0][:, a], tiles[1][:, b], tiles[2][:, c]
                ok = (tx >= 0) & (ty >= 0) & (tz >= 0)
                np.add.at(cnt, ((tz * nt[1] + ty) * nt[0] + tx)[ok], 1)
    assert L == tiles[0].shape[0]
    return cnt


def regime_fields(n, kind, X, periodic, xf, block=None):
    cnt = bins(n, kind, X, periodic, xf, block)
    full = np.nonzero(cnt)[0]
    return dict(max_bin=int(cnt.max()), bins_over_256=int((cnt > 256).sum()), bins_over_512=int((cnt > 512).sum()),
                scan_rounds=sorted({int(t) // 4096 for t in full}), ntiles=int(cnt.size), L_mod_4=int(np.asarray(X[0]).size % 4),
                counts=cnt, first_tile=int(full.min()) if full.size else -1, last_tile=int(full.max()) if full.size else -1)


def ulp_factor(n):
    """K of the derived bound |U - U_ref| <= K u max|u| (tests/test_ibm_regimes.py): 60 (max n_d + 2) + 70"""
    return 60 * (max(n) + 2) + 70


# ---- a body in prescribed rigid motion (fl_ibm_rigid_pose) ----------------------------------------------------------------------------------

U53 = 2.0 ** -53


def rigid_pose(X0, centre0, centre, rotvec, velocity, omega):
    """X_l = centre + R(rotvec) (X0_l - centre0) by Rodrigues' rotation of each vector, r' = r cos th + (k x r) sin th + k (k . r)(1 - cos th),
    rotvec = th k, and Ut_l = velocity + omega x (X_l - centre), in long double (1 - cos th as 2 sin^2(th / 2): no cancellation at a small angle).
    X0: (3, L).  -> X (3, L), Ut (3, L) long double and the bounds bX, bU (3, L) double a correctly built fp64 evaluation stays within:

    u = 2^-53.  The library forms the nine entries of R on the host in double: th = sqrt(sum of three squares), relative error <= 3 u; k = rotvec / th,
    <= 4 u; cos and sin of the rounded th, off by <= 3 u th from the argument and <= 2 u from the library: (3 th + 2) u each, absolutely.  An entry is
    [a == b] cos + sin K_ab + (1 - cos) k_a k_b, every factor at most 1 (1 - cos: 2) in size: (3 th + 7) u for the second term, (3 th + 24) u for the
    third (one subtraction and two products of values up to 2, 4 u twice for k), 3 u for the two additions -- (9 th + 36) u =: KR u per entry.
    On the device r0 = X0 - centre0 (u |r0_b| each), r_a = sum_b R_ab r0_b (a dot product of three: 3 u sum |R_ab r0_b|, fused or not), with |R_ab| <= 1:
        |r_a - exact| <= (KR + 1 + 3) u S0,   S0 = sum_b |r0_b|,   and |r_a| <= S0
    X_a = centre_a + r_a, one more rounding of a value <= |centre_a| + S0:             bX = ((KR + 5) S0 + |centre_a|) u
    Ut_a = v_a + (w_b r_c - w_c r_b): the products inherit r's error and round once, the difference and the sum round once each:
                                                                                        bU = ((KR + 7) (|w_b| + |w_c|) S0 + |v_a|) u
    both times 1 + 2^-10 for the terms of second order and this reference's own rounding (2^-64 relative per operation)."""
    X0 = np.asarray(X0, dtype=np.float64).astype(LD)
    c0, c, rv, v, w = [np.asarray(a, dtype=np.float64).astype(LD) for a in (centre0, centre, rotvec, velocity, omega)]
    th = np.sqrt(rv[0] * rv[0] + rv[1] * rv[1] + rv[2] * rv[2])
    r0 = X0 - c0[:, None]
    if th > 0:
        k = rv / th
        cs, sn, vers = np.cos(th), np.sin(th), 2 * np.sin(th / 2) ** 2
        kxr = np.stack([k[1] * r0[2] - k[2] * r0[1], k[2] * r0[0] - k[0] * r0[2], k[0] * r0[1] - k[1] * r0[0]])
        kr = k[0] * r0[0] + k[1] * r0[1] + k[2] * r0[2]
        r = r0 * cs + kxr * sn + k[:, None] * (kr * vers)[None, :]
    else:
        r = r0.copy()
    X = c[:, None] + r
    Ut = v[:, None] + np.stack([w[1] * r[2] - w[2] * r[1], w[2] * r[0] - w[0] * r[2], w[0] * r[1] - w[1] * r[0]])
    KR = 9.0 * float(th) + 36.0
    S0 = np.abs(r0).sum(axis=0).astype(np.float64)
    slack = 1 + 2.0 ** -10
    cabs, vabs, wabs = [np.abs(np.asarray(a, dtype=np.float64)) for a in (centre, velocity, omega)]
    bX = np.stack([((KR + 5) * S0 + cabs[a]) * U53 * slack for a in range(3)])
    bU = np.stack([((KR + 7) * (wabs[(a + 1) % 3] + wabs[(a + 2) % 3]) * S0 + vabs[a]) * U53 * slack for a in range(3)])
    return X, Ut, bX, bU


def rigid_pose_within(got, want, bound):
    """largest |got - want| / bound over the entries (long double difference; a zero bound admits only the exact value)"""
    err = np.abs(np.asarray(got, dtype=np.float64).astype(LD) - want).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(err == 0, 0.0, err / np.asarray(bound, dtype=np.float64))
    return float(q.max()) if q.size else 0.0
