"""-m gpu, one rank: fl_ibm_scalar_force / fl_ibm_scalar_rate (include/fluca_hip_ibm_scalar.h) on the grids and the marker set of
tests/ibm_scalar_cases.py -- a bin of two LDS chunks, supports through the periodic seam and cut by walls, markers on the lattice, an extent that
is no multiple of the tile, both delta functions, uniform and stretched.

The contract is bitwise: phi and Q against fl_ibm_interp(1) -> fl_vec_lincomb(-1 Phi + 1 T) -> fl_ibm_spread(1) per pass through the existing entry
points (Q accumulated by one double addition per pass).  Then the long-double reference of tests/ibm_scalar_reference.py within its derived bound,
what surrounds phi and Q, Q_dev = NULL, an empty set, the rate against fl_ibm_force and the numpy split sum, and conservation."""
import ctypes as C

import numpy as np
import pytest

from tests import ibm_scalar_cases as sc
from tests import ibm_scalar_reference as isr
from tests.test_gpu_ibm_regimes import Markers, dev, host

pytestmark = pytest.mark.gpu

KINDS = [0, 1]
GRIDS = pytest.mark.parametrize("uniform", [True, False], ids=["uniform", "stretched"])
PAD = 64                                   # sentinel doubles on either side of phi and Q


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def ints(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.int32), device="cuda")


class Pool:
    def __init__(self):
        self.P, self.sets = {}, {}

    def poisson(self, uniform):
        from fluca_amd.poisson import Poisson
        if uniform not in self.P:
            self.P[uniform] = Poisson(sc.N, sc.grid(uniform), sc.BC, 1e-3)
        return self.P[uniform]

    def markers(self, uniform, kind, groups=None):
        key = (uniform, kind, groups)
        if key not in self.sets:
            self.sets[key] = Markers(self.poisson(uniform), kind, sc.markers(groups))
        return self.sets[key]

    def close(self):
        for m in self.sets.values():
            m.close()
        for P in self.P.values():
            P.close()


@pytest.fixture(scope="module")
def pool():
    p = Pool()
    yield p
    p.close()


def padded(a, fill=np.nan):
    """a device array with PAD sentinels on either side, and the view of the middle"""
    import torch
    a = np.asarray(a, dtype=np.float64).ravel()
    buf = torch.full((a.size + 2 * PAD,), fill, dtype=torch.float64, device="cuda")
    buf[PAD:PAD + a.size] = dev(a)
    return buf, buf[PAD:PAD + a.size]


def fused(m, npass, dV, phi0, T=None, body=None, values=None, with_Q=True):
    """fl_ibm_scalar_force -> phi, Q (host), and whether the sentinels around both survived"""
    from fluca_amd.capi import check, lib
    pbuf, phi = padded(phi0, 7.0)
    qbuf, Q = padded(np.full(m.L, -3.0), 5.0)
    Td, bd, dVd = (dev(T) if T is not None else None), (ints(body) if body is not None else None), dev(dV)
    val = (C.c_double * len(values))(*values) if values is not None else None
    m.P._pre()
    check(lib.fl_ibm_scalar_force(m.h, npass, ptr(Td), ptr(bd), len(values) if values is not None else 1, val, ptr(dVd), ptr(phi), ptr(Q) if with_Q else None), "fl_ibm_scalar_force")
    if val is not None:
        for b in range(len(values)):
            val[b] = np.nan                 # the table was read before the call returned
    m.P._post()
    pb, qb = host(pbuf), host(qbuf)
    intact = bool(np.all(pb[:PAD] == 7.0) and np.all(pb[-PAD:] == 7.0) and np.all(qb[:PAD] == 5.0) and np.all(qb[-PAD:] == 5.0))
    return pb[PAD:-PAD].copy(), qb[PAD:-PAD].copy(), intact


def composition(m, npass, dV, phi0, T):
    """the three existing entry points per pass -> phi, Q (host)"""
    import torch
    from fluca_amd.capi import check, lib
    phi, Td, dVd = dev(phi0), dev(T), dev(dV)
    Q = None
    for k in range(npass):
        Phi = torch.full((m.L,), np.nan, dtype=torch.float64, device="cuda")
        q = torch.full((m.L,), np.nan, dtype=torch.float64, device="cuda")
        m.P._pre()
        check(lib.fl_ibm_interp(m.h, 1, ptr(phi), ptr(Phi)), "fl_ibm_interp")
        check(lib.fl_vec_lincomb(m.P.h, m.L, -1.0, ptr(Phi), 1.0, ptr(Td), ptr(q)), "fl_vec_lincomb")
        check(lib.fl_ibm_spread(m.h, 1, ptr(q), ptr(dVd), ptr(phi)), "fl_ibm_spread")
        m.P._post()
        Q = q.clone() if Q is None else Q + q
    return host(phi), host(Q)


_COMP = {}


def composed(pool, uniform, kind, npass, which):
    key = (uniform, kind, npass, which)
    if key not in _COMP:
        d = sc.data()
        _COMP[key] = composition(pool.markers(uniform, kind), npass, d["dV"], d["phi0"], d[which])
    return _COMP[key]


def same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.int64), np.asarray(b).view(np.int64))


@pytest.mark.parametrize("npass", sc.NPASSES)
@pytest.mark.parametrize("kind", KINDS)
@GRIDS
def test_phi_and_Q_are_the_bits_of_the_composition(uniform, kind, npass, pool):
    """with a target per marker, and with a value per body on three interleaved bodies; Q_dev = NULL gives the same phi; sentinels keep their bits"""
    m, d = pool.markers(uniform, kind), sc.data()
    phi_c, Q_c = composed(pool, uniform, kind, npass, "T")
    phi, Q, intact = fused(m, npass, d["dV"], d["phi0"], T=d["T"])
    assert intact and same_bits(phi, phi_c) and same_bits(Q, Q_c)
    assert not np.array_equal(phi, d["phi0"])
    phi_n, Q_n, intact = fused(m, npass, d["dV"], d["phi0"], T=d["T"], with_Q=False)
    assert intact and same_bits(phi_n, phi_c) and np.all(Q_n == -3.0)
    phi_c, Q_c = composed(pool, uniform, kind, npass, "Tbody")
    phi, Q, intact = fused(m, npass, d["dV"], d["phi0"], body=d["body"], values=sc.VALUES)
    assert intact and same_bits(phi, phi_c) and same_bits(Q, Q_c)


@pytest.mark.parametrize("kind", KINDS)
def test_one_body_needs_no_ids(kind, pool):
    m, d = pool.markers(True, kind), sc.data()
    phi_c, Q_c = composition(m, 2, d["dV"], d["phi0"], np.full(m.L, 0.75))
    phi, Q, intact = fused(m, 2, d["dV"], d["phi0"], values=[0.75])
    assert intact and same_bits(phi, phi_c) and same_bits(Q, Q_c)


@pytest.mark.parametrize("npass", sc.NPASSES)
@pytest.mark.parametrize("kind", KINDS)
@GRIDS
def test_phi_and_Q_are_within_the_derived_bound_of_the_long_double_reference(uniform, kind, npass, pool):
    """... and the cells outside every support keep their bits"""
    m, d = pool.markers(uniform, kind), sc.data()
    geo = isr.Geometry(sc.N, sc.grid(uniform), sc.PERIODIC, kind, sc.markers())
    phi_r, Q_r, qs, phis = isr.force(geo, d["T"], d["dV"], d["phi0"], npass)
    bphi, bQ = isr.bounds(geo, d["T"], d["dV"], qs, phis)
    phi, Q, _ = fused(m, npass, d["dV"], d["phi0"], T=d["T"])
    ephi = float(np.abs(phi.astype(isr.LD) - phi_r).max())
    eQ = float(np.abs(Q.astype(isr.LD) - Q_r).max())
    print(f"uniform {uniform} kind {kind} npass {npass}: phi {ephi:.2e} of {bphi:.2e}, Q {eQ:.2e} of {bQ:.2e}")
    assert ephi <= bphi and eQ <= bQ
    out = ~geo.reached()
    assert out.any() and same_bits(phi[out], d["phi0"][out])


@pytest.mark.parametrize("kind", KINDS)
def test_an_owned_set_without_markers_is_success_and_changes_nothing(kind, pool):
    """L = 0 (fl_ibm_create_owned on one rank with no marker): no launch, phi keeps its bits, the rate is zero"""
    from fluca_amd.capi import check, lib
    P, d = pool.poisson(True), sc.data()
    h = C.c_void_p()
    P._pre()
    check(lib.fl_ibm_create_owned(P.h, kind, 0, None, None, None, None, C.byref(h)), "fl_ibm_create_owned")
    phi = dev(d["phi0"])
    v = (C.c_double * 3)(*sc.VALUES)
    check(lib.fl_ibm_scalar_force(h, 3, None, None, 3, v, None, ptr(phi), None), "fl_ibm_scalar_force (L = 0)")
    check(lib.fl_ibm_scalar_force(h, 3, None, None, 1, None, None, ptr(phi), None), "fl_ibm_scalar_force (L = 0, no target)")
    rate = (C.c_double * 3)(9.0, 9.0, 9.0)
    check(lib.fl_ibm_scalar_rate(h, None, None, None, 3, rate), "fl_ibm_scalar_rate (L = 0)")
    P._post()
    assert same_bits(host(phi), d["phi0"]) and list(rate) == [0.0, 0.0, 0.0]
    lib.fl_ibm_destroy(h)


@pytest.mark.parametrize("kind", KINDS)
def test_a_set_without_an_active_tile_changes_nothing(kind, pool):
    """five markers whose supports lie wholly beyond the low x wall: no tile is launched, Phi = 0, so q = T in every pass and phi keeps its bits"""
    d = sc.data()
    rng = np.random.default_rng(75)
    X = [np.full(5, sc.BOX[0][0] - 5.0 * sc.H), rng.uniform(0.3, 0.9, 5), rng.uniform(0.2, 0.8, 5)]
    m = Markers(pool.poisson(True), kind, X)
    T, dV = rng.standard_normal(5), np.full(5, sc.H ** 3)
    phi, Q, intact = fused(m, 2, dV, d["phi0"], T=T)
    phi_c, Q_c = composition(m, 2, dV, d["phi0"], T)
    m.close()
    assert intact and same_bits(phi, d["phi0"]) and same_bits(phi_c, d["phi0"]) and same_bits(Q, Q_c) and same_bits(Q, T + T)


def test_argument_errors_on_a_set(pool):
    from fluca_amd.capi import lib
    m, d = pool.markers(True, 0), sc.data()
    phi, T, dV, body = dev(d["phi0"]), dev(d["T"]), dev(d["dV"]), ints(d["body"])
    v = (C.c_double * 3)(*sc.VALUES)
    m.P._pre()
    f = lib.fl_ibm_scalar_force
    assert f(m.h, 1, ptr(T), None, 1, None, ptr(dV), None, None) == -85                # FL_ERR_ARG_NULL: phi
    assert f(m.h, 1, ptr(T), None, 1, None, None, ptr(phi), None) == -85               # dV
    assert f(m.h, 0, ptr(T), None, 1, None, ptr(dV), ptr(phi), None) == -63            # FL_ERR_ARG_OUTOFRANGE: npass
    assert f(m.h, 17, ptr(T), None, 1, None, ptr(dV), ptr(phi), None) == -63
    assert f(m.h, 1, None, ptr(body), 0, v, ptr(dV), ptr(phi), None) == -63            # nbody
    assert f(m.h, 1, None, ptr(body), 65, v, ptr(dV), ptr(phi), None) == -63
    assert f(m.h, 1, ptr(T), ptr(body), 3, v, ptr(dV), ptr(phi), None) == -62          # FL_ERR_ARG_WRONG: both
    assert f(m.h, 1, None, ptr(body), 3, None, ptr(dV), ptr(phi), None) == -62         # neither
    r = (C.c_double * 3)(9.0, 9.0, 9.0)
    g = lib.fl_ibm_scalar_rate
    assert g(m.h, None, ptr(dV), ptr(body), 3, r) == -85 and g(m.h, ptr(T), ptr(dV), ptr(body), 3, None) == -85
    assert g(m.h, ptr(T), ptr(dV), ptr(body), 0, r) == -63 and g(m.h, ptr(T), ptr(dV), ptr(body), 65, r) == -63
    assert g(m.h, ptr(T), ptr(dV), ptr(body), 2, r) == -63                             # an id outside 0..nbody-1, as fl_ibm_force
    m.P._post()
    assert same_bits(host(phi), d["phi0"]) and list(r) == [9.0, 9.0, 9.0]


def _force_first(m, Q, dV, body, nbody):
    """fl_ibm_force's force[3 b] for F = (Q, 0, 0)"""
    from fluca_amd.capi import check, lib
    F = dev(np.concatenate([Q, np.zeros(2 * Q.size)]))
    dVd, bd = dev(dV), (ints(body) if body is not None else None)
    about, force = (C.c_double * (3 * nbody))(), (C.c_double * (3 * nbody))()
    m.P._pre()
    check(lib.fl_ibm_force(m.h, ptr(F), ptr(dVd), ptr(bd), nbody, about, force, None), "fl_ibm_force")
    m.P._post()
    return np.array(list(force)).reshape(nbody, 3)[:, 0]


def _rate(m, Q, dV, body, nbody):
    from fluca_amd.capi import check, lib
    Qd, dVd, bd = dev(Q), dev(dV), (ints(body) if body is not None else None)
    rate = (C.c_double * nbody)()
    m.P._pre()
    check(lib.fl_ibm_scalar_rate(m.h, ptr(Qd), ptr(dVd), ptr(bd), nbody, rate), "fl_ibm_scalar_rate")
    m.P._post()
    return np.array(list(rate))


@pytest.mark.parametrize("kind", KINDS)
def test_rate_is_fl_ibm_force_and_the_split_sum(kind, pool):
    """the Q of a forcing call, and a Q over twelve decades: fl_ibm_force's first components bit for bit, the numpy split sum's bits, the same bits
    from a set that holds the markers in another order; one body without ids; a non-finite Q is a NaN group and success"""
    m, d = pool.markers(True, kind), sc.data()
    _, Q, _ = fused(m, 2, d["dV"], d["phi0"], body=d["body"], values=sc.VALUES)
    rng = np.random.default_rng(74)
    wide = rng.standard_normal(m.L) * 10.0 ** rng.integers(-6, 6, m.L)
    X = sc.markers()
    p = rng.permutation(m.L)
    mp = Markers(pool.poisson(True), kind, [a[p] for a in X])
    for q in (Q, wide):
        got = _rate(m, q, d["dV"], d["body"], 3)
        assert same_bits(got, _force_first(m, q, d["dV"], d["body"], 3))
        assert same_bits(got, isr.rate(q, d["dV"], d["body"], 3))
        assert same_bits(got, _rate(mp, q[p], d["dV"][p], d["body"][p], 3))
        one = _rate(m, q, d["dV"], None, 1)
        assert same_bits(one, isr.rate(q, d["dV"])) and same_bits(one, _force_first(m, q, d["dV"], None, 1))
    mp.close()
    bad = wide.copy()
    bad[11] = np.inf
    assert np.isnan(_rate(m, bad, d["dV"], d["body"], 3)).all()


@pytest.mark.parametrize("npass", (1, 5))
@pytest.mark.parametrize("kind", KINDS)
@GRIDS
def test_the_field_gains_what_the_markers_hand_out(uniform, kind, npass, pool):
    """markers at least two cells from the walls: sum_c dphi_c vol_c = sum_l Q_l dV_l = the sum of the rates, to the reference's margin"""
    m, d = pool.markers(uniform, kind, sc.INNER), sc.data(sc.INNER)
    phi, Q, _ = fused(m, npass, d["dV"], d["phi0"], body=d["body"], values=sc.VALUES)
    lhs, rhs, margin = sc.conservation(sc.grid(uniform), d["phi0"], phi, Q, d["dV"])
    total = float(_rate(m, Q, d["dV"], d["body"], 3).sum())
    print(f"uniform {uniform} kind {kind} npass {npass}: {lhs:.15e} {rhs:.15e} {total:.15e} margin {margin:.1e}")
    assert abs(lhs - rhs) <= margin and abs(lhs - total) <= margin and abs(rhs) > 1e3 * margin
