"""-m gpu: whole SEQUENCES of calls on one handle queued behind ONE delay, with no host wait in between -- what a time step looks like to the GPU
when the host runs hundreds of launches ahead.  tests/test_gpu_caller_arrays.py makes every entry point once behind a delay; what it cannot show is
a call reaching back into a queued earlier one: a table refreshed in place while a queued kernel still needs the old one, a setter that changes a
launch already made, a host buffer rewritten before its copy has left, an output written on a side stream that is not joined back.

Every test plays its sequence twice on the same handle (play below): IDLE -- call by call, the stream drained after every call, every input
complete -- and QUEUED -- a delay (tests/stream_order.py: DELAY_MS of torch.cuda._sleep) goes onto the handle's stream first, then the producers of
all inputs (device-to-device copies through staging tensors; until they run the arrays hold poison), then the calls, the snapshots (clones in stream
order) and the poisoning of every array the caller is free to reuse, all without a host wait.  Where the sequence has made only calls that
tests/stream_order.py classes `async`, S.still_pending() asserts that the delay had not ended: nothing has run yet, and no call waited.  Every snapshot
of the queued run must be finite and have the idle run's bits (a repeat on one handle is bitwise the same: tests/test_gpu_handle_history.py); the idle
values are held to the oracle where that is cheap, so that the sequence is known to compute what it says.

Copied arrays (fl_momentum_set_state*, fl_ibm_update) are poisoned as soon as the call has returned; borrowed ones (fl_scalar_set_velocity) after the
last call the header lets read them; the pinned source of fl_poisson_upload after fl_poisson_upload_fence.  Poison is NaN, except for marker
positions -- they become cell indices: another valid marker set -- and host arrays of pointers, which are redirected to a decoy device array.

Grids: G2 (12, 9, 5) cavity and G3 (130, 9, 3) channel of tests/test_gpu_caller_arrays.py: the smallest where k_mom3, a second 128-cell segment and
the outlet rows are live; CG + multigrid with three levels on (32, 32, 16).

Which calls wait and which arrays are copied or borrowed: include/fluca_hip.h ("Stream order") and tests/stream_order.py say the same.  Not run
here: the owner-rank marker calls fl_ibm_owned_select / create_owned / migrate (collective, they wait by design) and fl_ibm_owned_fetch."""
import ctypes as C
import time

import numpy as np
import pytest
import torch

from oracle import fluca_oracle as fo
from tests import inproc
from tests import scalar_cases as sc
from tests import scalar_ranks as rk
from tests import stream_order as so
from tests.gpu_common import PER, O, V, dev, make_pair, mean_free_rhs
from tests.test_gpu_caller_arrays import GAMMA, GRIDS, SCALAR_BC, bits, ptr, ptrs, same_bits

pytestmark = pytest.mark.gpu

TWO = pytest.mark.parametrize("gname", ["G2", "G3"])
NAN = float("nan")


# ------------------------------------------------------------------------------------------------------------------ the harness

class Session:
    """the arrays of one play: S[name]; inputs hold poison until produce() has run on the stream"""

    def __init__(self, P, inputs, outs, poison, queued):
        self.P, self.queued = P, queued
        self.src = {n: dev(np.asarray(a, dtype=np.float64).reshape(-1)) for n, a in inputs.items()}
        self.poison = {n: (dev(np.asarray(poison[n], dtype=np.float64).reshape(-1)) if n in poison else torch.full_like(t, NAN)) for n, t in self.src.items()}
        self.stage = {n: self.poison[n].clone() for n in self.src}        # complete only once produce() has run on the stream, like the arrays
        self.t = {n: self.poison[n].clone() for n in self.src}
        for n, l in outs.items():                               # an output starts as NaN, or as the valid values the case names (what becomes an index)
            if np.ndim(l):
                self.poison[n] = dev(np.asarray(l, dtype=np.float64).reshape(-1))
                self.t[n] = self.poison[n].clone()
            else:
                self.t[n] = torch.full((int(l),), NAN, dtype=torch.float64, device="cuda")
        self.snaps, self.hosts, self.e, self.t0, self.asserted = {}, {}, None, None, 0

    def __getitem__(self, name):
        return self.t[name]

    def produce(self):
        for n, src in self.src.items():
            self.stage[n].copy_(src)
        for n in self.src:                                      # the producer proper: a copy that ran on another stream would hand on the staging poison
            self.t[n].copy_(self.stage[n])
        self.tick()

    def tick(self):
        """idle: drain the stream after a call.  queued: nothing"""
        if not self.queued:
            self.P.stream.synchronize()

    def do(self, f, *a, **kw):
        r = f(*a, **kw)
        self.tick()
        return r

    def raw(self, fn, *args):
        from fluca_amd import capi
        rc = getattr(capi.lib, fn)(*args)
        assert rc == 0, (fn, rc)
        self.tick()

    def snap(self, key, what):
        """clone an array (or a list of them) in stream order"""
        ts = [self.t[w] if isinstance(w, str) else w for w in (what if isinstance(what, (list, tuple)) else [what])]
        self.snaps[key] = [t.clone() for t in ts]
        self.tick()

    def host(self, key, value):
        self.hosts[key] = np.array(value, dtype=np.float64)

    def release(self, *names):
        """the caller reuses these buffers: poison, in stream order, in both plays"""
        for n in names:
            self.t[n].copy_(self.poison[n]) if n in self.poison else self.t[n].fill_(NAN)
        self.tick()

    def ended(self):
        return self.e is not None and self.e.query()

    def still_pending(self, what):
        """only `async` calls so far: the delay must not have ended (else a call waited, or the play proves nothing)"""
        if self.queued and self.e is not None:
            ended, ms = self.e.query(), (time.perf_counter() - self.t0) * 1e3
            print(f"{what}: {ms:.3f} ms of host time since the delay was queued, the delay had {'ENDED' if ended else 'not ended'}")
            assert not ended, (what, f"{ms:.3f} ms on the host: a call that must only enqueue waited for the {so.DELAY_MS} ms delay")
            self.asserted += 1

    def results(self):
        out = {k: [t.cpu().numpy().copy() for t in ts] for k, ts in self.snaps.items()}
        out.update({k: [v] for k, v in self.hosts.items()})
        return out


def play(P, seq, inputs, outs, poison=None, queued=False, delay=True):
    S = Session(P, inputs, outs, poison or {}, queued)
    torch.cuda.synchronize()
    with torch.cuda.stream(P.stream):
        if queued and delay:
            S.e = so.Delay.queue()
        S.t0 = time.perf_counter()
        S.produce()
        seq(S)
    P.stream.synchronize()
    return S.results(), S


def both(label, P, seq, inputs, outs, poison=None, delay=True, must_assert=True, before=None):
    """-> the idle results; the queued ones are held to their bits.  before(): puts the handle into the state both plays start from"""
    if before is not None:
        before()
    idle = play(P, seq, inputs, outs, poison, queued=False)[0]     # (its arrays go back to the allocator: the queued play allocates nothing new)
    if before is not None:
        before()
    got, S = play(P, seq, inputs, outs, poison, queued=True, delay=delay)
    assert sorted(got) == sorted(idle) and idle, label
    bad = []
    for k in idle:
        for i, (a, b) in enumerate(zip(idle[k], got[k])):
            assert np.isfinite(a).all() and np.isfinite(b).all(), (label, k, i, "not finite")
            if not same_bits(a, b):
                w = np.flatnonzero(bits(a).ravel() != bits(b).ravel())
                bad.append((k, i, int(w.size), int(w[0]), float(a.ravel()[w[0]]), float(b.ravel()[w[0]])))
    print(f"{label}: {sum(len(v) for v in idle.values())} snapshots, queued = idle bit for bit: {not bad}")
    assert not bad, (label, "the queued sequence differs from the idle one (key, part, entries, first entry, idle, queued)", bad)
    assert not (must_assert and delay) or S.asserted > 0, (label, "the sequence never asserted that the delay was pending")
    return idle


def differ(a, b):
    return not same_bits(a, b)


@pytest.fixture(scope="module")
def pairs():
    made = {}

    def get(name):
        if name not in made:
            n, bc = GRIDS[name]
            made[name] = make_pair(n, bc, kappa=1e-3) + (n, bc)
        return made[name]
    yield get
    for P, g, n, bc in made.values():
        P.close()


def close_to(got, want, tol=2e-13):
    assert np.abs(got - want).max() <= tol * np.abs(want).max(), (np.abs(got - want).max(), np.abs(want).max())


# ------------------------------------------------------------------------------------------------------------------ momentum

@TWO
def test_momentum_three_states_in_a_row(pairs, gname):
    """set_state(S1) apply diagonal | set_state(S2) apply | set_state_v0(S3) apply | set_coefficients(0, 1, 0) apply | fl_momentum_rhs (which scales
    the tables of slot 1) | apply.  Three states in a row: a table double-buffered one deep would hand the first product the third state's rows."""
    from fluca_amd.poisson import Momentum
    P, g, n, bc = pairs(gname)
    M = Momentum(P)
    N, nf = g.ncell, [int(a) for a in g.nface]
    rng = np.random.default_rng(101)
    mu, rho = 0.05, 1.0
    dts = [g.kappa * rho, 0.7 * g.kappa * rho, 1.3 * g.kappa * rho]
    st = []
    for s in range(3):
        V0 = [4.0 * rng.standard_normal(nf[d]) for d in range(3)]
        if s < 2:
            W = [4.0 * rng.standard_normal(nf[q % 3]) for q in range(9)]
            v0 = None
        else:
            v0 = rng.standard_normal(3 * N)
            W = g.apply_B(v0)
        st.append((V0, W, v0))
    v = rng.standard_normal(3 * N)
    dt_r, rho_r, mu_r = 0.013, 13.0, 0.4                        # dt / rho = the handle's kappa
    v0r, pr, vbc = rng.standard_normal(3 * N), rng.standard_normal(N), rng.standard_normal(3 * N)
    inputs = {"v": v, "v0r": v0r, "p": pr, "vbc": vbc}
    for s, (V0, W, v0) in enumerate(st):
        inputs.update({f"V0{s}{d}": V0[d] for d in range(3)})
        inputs.update({f"W{s}{q}": W[q] for q in range(9)})
    inputs["v03"] = st[2][2]
    outs = {"y": 3 * N, "d": 3 * N, "r": 3 * N}

    def state(S, s):
        names = [f"V0{s}{d}" for d in range(3)] + [f"W{s}{q}" for q in range(9)] + (["v03"] if s == 2 else [])
        S.do(M.set_state, dts[s], rho, mu, [S[f"V0{s}{d}"] for d in range(3)], [S[f"W{s}{q}"] for q in range(9)], v0=S["v03"] if s == 2 else None)
        S.release(*names)                                       # copied: the caller reuses its buffers at once

    def seq(S):
        state(S, 0)
        S.do(M.apply, S["v"], S["y"]); S.snap("y1", "y")
        S.raw("fl_momentum_diagonal", M.h, ptr(S["d"])); S.snap("d1", "d")
        state(S, 1)
        S.do(M.apply, S["v"], S["y"]); S.snap("y2", "y")
        state(S, 2)
        S.do(M.apply, S["v"], S["y"]); S.snap("y3", "y")
        S.do(M.set_coefficients, 0.0, 1.0, 0.0)
        S.do(M.apply, S["v"], S["y"]); S.snap("y4", "y")
        S.do(M.rhs, dt_r, rho_r, mu_r, S["v0r"], S["p"], S["vbc"], out=S["r"]); S.snap("r", "r")
        S.do(M.apply, S["v"], S["y"]); S.snap("y5", "y")
        S.still_pending(f"{gname} momentum: 4 states and coefficient sets, 5 products, diagonal, rhs")
        S.release("v", "v0r", "p", "vbc")
    try:
        idle = both(f"{gname} momentum sequence", P, seq, inputs, outs)
    finally:
        M.close()
    y = {k: idle[k][0] for k in idle}
    assert same_bits(y["y5"], y["y4"]), "fl_momentum_rhs changed the operator of the next product"
    assert differ(y["y1"], y["y2"]) and differ(y["y2"], y["y3"]) and differ(y["y3"], y["y4"])
    for s, key in ((0, "y1"), (1, "y2")):                       # tests/test_gpu_momentum.py::_close
        A = g.assemble_momentum(1.0, dts[s], -0.5 * mu * dts[s] / rho, st[s][0], st[s][1])
        close_to(y[key], A.mult(v))
        if s == 0:
            close_to(y["d1"], A.diag())
    A3 = g.assemble_momentum(1.0, dts[2], -0.5 * mu * dts[2] / rho, st[2][0], st[2][1])
    close_to(y["y3"], A3.mult(v))
    close_to(y["y4"], g.assemble_momentum(0.0, 1.0, 0.0, st[2][0], st[2][1]).mult(v))


# ------------------------------------------------------------------------------------------------------------------ Poisson

def pinned(n):
    from fluca_amd import capi
    p = C.c_void_p()
    capi.check(capi.lib.fl_malloc_host(8 * n, C.byref(p)), "fl_malloc_host")
    return p, np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_double)), (n,))


@TWO
def test_poisson_sequence_with_two_uploads_into_one_plane(pairs, gname):
    """apply, rhs, project (six), project (subset), pressure_update first and later, gst_bc, the three fl_boundary_* calls; the SAME device plane is
    filled by fl_poisson_upload from one pinned buffer, added, filled from a second pinned buffer, added again.  fl_poisson_upload_fence then returns
    only after the delay, and rewriting both host buffers after it changes nothing."""
    from fluca_amd import capi
    P, g, n, bc = pairs(gname)
    N, nf = g.ncell, [int(a) for a in g.nface]
    rng = np.random.default_rng(202)
    b = 1                                                       # high x: the outlet of G3, a wall of G2
    m = n[1] * n[2]
    Vf = [rng.standard_normal(nf[d]) for d in range(3)]
    inputs = {"x": rng.standard_normal(N), "cr": rng.standard_normal(N), "p": rng.standard_normal(N), "dp": rng.standard_normal(N), "p0": rng.standard_normal(N),
              "pb": rng.standard_normal(m), "plane": rng.standard_normal(m), "F": rng.standard_normal(nf[0]), "G": rng.standard_normal(nf[0]), "Cc": rng.standard_normal(N),
              "H": rng.standard_normal(nf[0]), **{f"Vr{d}": Vf[d] for d in range(3)}, **{f"v{d}": rng.standard_normal(N) for d in range(3)},
              **{f"V{d}": rng.standard_normal(nf[d]) for d in range(3)}}
    outs = {"y": N, "b": N, "phalf": N, "pp": N, "up": m}
    h1, a1 = pinned(m)
    h2, a2 = pinned(m)
    up1, up2 = rng.standard_normal(m), rng.standard_normal(m)
    coeff = -1.37
    state = {}

    def seq(S):
        a1[:], a2[:] = up1, up2
        S.do(P.apply, S["x"], S["y"]); S.snap("a", "y")
        S.do(P.rhs, S["Vr0"], S["Vr1"], S["Vr2"], contrhs=S["cr"], b=S["b"]); S.snap("b", "b")
        S.do(P.project, S["p"], v=[S[f"v{d}"] for d in range(3)], V=[S[f"V{d}"] for d in range(3)]); S.snap("c", [f"v{d}" for d in range(3)] + [f"V{d}" for d in range(3)])
        S.do(P.project, S["p"], v=[S["v0"], None, None], V=[None, S["V1"], None]); S.snap("d", ["v0", "V1", "v1", "V0"])
        S.do(P.pressure_update, True, S["dp"], S["p0"], S["phalf"], S["pp"]); S.snap("pu1", ["phalf", "pp"])
        S.do(P.pressure_update, False, S["dp"], None, S["phalf"], S["pp"]); S.snap("pu2", ["phalf", "pp"])
        S.raw("fl_poisson_gst_bc", P.h, b, ptr(S["pb"]), ptr(S["G"])); S.snap("gst", "G")
        S.raw("fl_boundary_set_faces", P.h, b, coeff, ptr(S["plane"]), ptr(S["F"])); S.snap("set", "F")
        S.raw("fl_boundary_add_cells", P.h, b, coeff, ptr(S["plane"]), ptr(S["Cc"])); S.snap("addc", "Cc")
        S.raw("fl_poisson_upload", P.h, ptr(S["up"]), h1, 8 * m)
        S.raw("fl_boundary_add_faces", P.h, b, coeff, ptr(S["up"]), ptr(S["H"])); S.snap("add1", "H")
        S.raw("fl_poisson_upload", P.h, ptr(S["up"]), h2, 8 * m)
        S.raw("fl_boundary_add_faces", P.h, b, 2.0, ptr(S["up"]), ptr(S["H"])); S.snap("add2", ["H", "up"])
        S.still_pending(f"{gname} Poisson: apply, rhs, 2 projections, 2 pressure updates, gst_bc, 4 boundary calls, 2 uploads")
        S.release("x", "cr", "p", "dp", "p0", "pb", "plane", "Vr0", "Vr1", "Vr2")
        capi.check(capi.lib.fl_poisson_upload_fence(P.h), "fl_poisson_upload_fence")
        if S.queued:
            state["fence_after_delay"] = S.ended()
        a1[:], a2[:] = NAN, NAN                                 # the fence has returned: the host buffers are the caller's again
    try:
        idle = both(f"{gname} Poisson sequence", P, seq, inputs, outs)
        assert state["fence_after_delay"], "fl_poisson_upload_fence returned while the delay in front of the uploads was still running"
    finally:
        capi.lib.fl_poisson_synchronize(P.h)
        capi.lib.fl_free_host(h1)
        capi.lib.fl_free_host(h2)
    S_ = g.assemble_S()
    x = inputs["x"]
    assert abs(idle["a"][0] - S_.mult(x)).max() <= 1e-13 * abs(S_.arrays()[2]).max() * 7 * abs(x).max()
    want_b = g.rhs(*Vf, contrhs=inputs["cr"])
    assert abs(idle["b"][0] - want_b).max() <= 1e-12 * max(1.0, abs(want_b).max())
    assert same_bits(idle["add2"][1], up2), "the plane does not hold the second upload"
    shp = (n[2], n[1], nf[0] // (n[1] * n[2]))
    H0, H2 = inputs["H"].reshape(shp), idle["add2"][0].reshape(shp)
    want = H0[:, :, -1] + coeff * up1.reshape(shp[:2]) + 2.0 * up2.reshape(shp[:2])
    assert np.abs(H2[:, :, -1] - want).max() <= 8 * 2.0 ** -53 * (np.abs(H0[:, :, -1]) + abs(coeff) * np.abs(up1.reshape(shp[:2])) + 2 * np.abs(up2.reshape(shp[:2]))).max()
    assert same_bits(H2[:, :, :-1], H0[:, :, :-1])
    assert same_bits(idle["pu1"][1], 2.0 * inputs["dp"] + inputs["p0"]) and same_bits(idle["pu2"][0], (inputs["dp"] + inputs["p0"]) + inputs["dp"])


# ------------------------------------------------------------------------------------------------------------------ scalar, one rank

@TWO
def test_scalar_setters_between_queued_launches(gname):
    """set_velocity(V1) rhs | new boundary value, limiter and diffusivity, rhs | set_velocity(V2) step (5 stages) | rhs.  A setter between two queued
    launches must not reach back into the first; V1 is the caller's again once V2 is set and the launches that read V1 are queued before its poison."""
    from tests import scalar_reference as sref
    n, bcname = GRIDS[gname][0], SCALAR_BC[gname]
    Pz, Sc = sc.make_handles(n, True, bcname, limiter="superbee", gamma=GAMMA)
    kinds, vals = sc.BC_SETS[bcname]
    V1 = sc.velocity(n, bcname)
    V2 = sc.velocity(n, bcname, seed=5)
    phi = sc.phi_field(n, "random") * 0.5 + sc.phi_field(n, "step")
    q = sc.source(n)
    N = phi.size
    Pr = sref.Problem(sc.faces(n, True), kinds, vals, GAMMA, "superbee")
    adv, dif = sref.cfl(Pr, V2, 1.0)
    dt = 0.5 / (adv + dif)
    side = kinds.index(sref.DIRICHLET) if sref.DIRICHLET in kinds else kinds.index(sref.NEUMANN)
    inputs = {"phi": phi, "q": q, **{f"A{d}": V1[d] for d in range(3)}, **{f"B{d}": V2[d] for d in range(3)}}
    outs = {"R": N}

    def seq(S):
        Sc.set_velocity(S["A0"], S["A1"], S["A2"])
        S.do(Sc.rhs, S["phi"], S["q"], out=S["R"]); S.snap("r1", "R")
        Sc.set_boundary_value(side, vals[side] + 0.625)
        Sc.set_limiter("minmod")
        Sc.set_diffusivity(2.0 * GAMMA)
        S.do(Sc.rhs, S["phi"], S["q"], out=S["R"]); S.snap("r2", "R")
        Sc.set_velocity(S["B0"], S["B1"], S["B2"])
        S.release("A0", "A1", "A2")                             # borrowed until the next set_velocity: behind the launches that read it
        S.do(Sc.step, S["phi"], dt, 5, S["q"]); S.snap("phi", "phi")
        S.do(Sc.rhs, S["phi"], S["q"], out=S["R"]); S.snap("r3", "R")
        S.still_pending(f"{gname} scalar: 3 x rhs, 5 stages, 2 x set_velocity, 3 setters")
        S.release("B0", "B1", "B2", "q")
        Sc.set_boundary_value(side, vals[side])                 # the handle as the next play expects it
        Sc.set_limiter("superbee")
        Sc.set_diffusivity(GAMMA)
    try:
        idle = both(f"{gname} scalar sequence", Pz, seq, inputs, outs)
    finally:
        Sc.close()
        Pz.close()
    want, E, _ = sref.rhs(Pr, phi, V1, q, np.longdouble, bounds=True, limiter="superbee")           # tests/test_gpu_scalar.py:58-65
    err = np.abs(idle["r1"][0].reshape(phi.shape).astype(np.longdouble) - want).astype(np.float64)
    assert (err <= sc.rhs_slack(E)).all(), float((err / sc.rhs_slack(E)).max())
    vals2 = list(vals)
    vals2[side] += 0.625
    Pr2 = sref.Problem(sc.faces(n, True), kinds, tuple(vals2), 2.0 * GAMMA, "minmod")
    want2, E2, _ = sref.rhs(Pr2, phi, V1, q, np.longdouble, bounds=True, limiter="minmod")
    err2 = np.abs(idle["r2"][0].reshape(phi.shape).astype(np.longdouble) - want2).astype(np.float64)
    assert (err2 <= sc.rhs_slack(E2)).all(), float((err2 / sc.rhs_slack(E2)).max())
    assert differ(idle["r1"][0], idle["r2"][0]) and differ(idle["r2"][0], idle["r3"][0])


# ------------------------------------------------------------------------------------------------------------------ immersed boundary

@TWO
def test_ibm_pose_update_interp_force(gname):
    """interp, spread, fl_ibm_rigid_pose (all three enqueue and return), then fl_ibm_update on the posed markers (waits), interp on the moved set,
    fl_ibm_force (host values).  The reference positions become cell indices two calls later: their poison is another marker set inside the box."""
    from fluca_amd import capi
    from tests import ibm_reference as ir
    from tests.test_gpu_caller_arrays import IBM_BC
    from tests.test_gpu_ibm import sphere_markers
    n, bc = GRIDS[gname][0], IBM_BC[gname]
    P, g = make_pair(n, bc, box=[(0.0, 1.0)] * 3)
    N, L, kind = g.ncell, 37, fo.DELTA_PESKIN4
    X0 = sphere_markers(L, (0.5, 0.5, 0.5), 0.3)
    other = sphere_markers(L, (0.45, 0.55, 0.5), 0.22, seed=1)
    rng = np.random.default_rng(303)
    u, F, dV, f0 = rng.standard_normal((3, N)), rng.standard_normal((3, L)), rng.uniform(0.5, 1.5, L) * 1e-3, rng.standard_normal((3, N))
    c0, c, vel, om = [0.5, 0.5, 0.5], [0.52, 0.49, 0.51], [0.3, -0.2, 0.1], [1.5, -2.0, 0.75]
    rotvec = list(np.array([2.0, -1.0, 2.0]) / 3.0 * 0.4)
    about = (C.c_double * 3)(0.5, 0.4375, 0.25)
    vec = lambda a: (C.c_double * 3)(*a)
    h = C.c_void_p()
    first = [dev(a) for a in X0]
    capi.check(capi.lib.fl_ibm_create(P.h, kind, L, ptr(first[0]), ptr(first[1]), ptr(first[2]), C.byref(h)), "fl_ibm_create")
    P.synchronize()
    inputs = {"X00": X0[0], "X01": X0[1], "X02": X0[2], "u": u, "F": F, "dV": dV, "f": f0}
    poison = {"X00": other[0], "X01": other[1], "X02": other[2]}
    outs = {"U": 3 * L, "X": other[0], "Y": other[1], "Z": other[2], "Ut": 3 * L}       # fl_ibm_update reads X, Y, Z: never a NaN there

    def seq(S):
        S.raw("fl_ibm_interp", h, 3, ptr(S["u"]), ptr(S["U"])); S.snap("U1", "U")
        S.raw("fl_ibm_spread", h, 3, ptr(S["F"]), ptr(S["dV"]), ptr(S["f"])); S.snap("f1", "f")
        S.raw("fl_ibm_rigid_pose", P.h, L, ptr(S["X00"]), ptr(S["X01"]), ptr(S["X02"]), vec(c0), vec(c), vec(rotvec), vec(vel), vec(om),
              ptr(S["X"]), ptr(S["Y"]), ptr(S["Z"]), ptr(S["Ut"])); S.snap("pose", ["X", "Y", "Z", "Ut"])
        S.still_pending(f"{gname} IBM: interp, spread, rigid_pose")
        S.release("X00", "X01", "X02")
        S.raw("fl_ibm_update", h, ptr(S["X"]), ptr(S["Y"]), ptr(S["Z"]))
        S.release("X", "Y", "Z")                                # copied into the set
        S.raw("fl_ibm_interp", h, 3, ptr(S["u"]), ptr(S["U"])); S.snap("U2", "U")
        force, torque = (C.c_double * 3)(), (C.c_double * 3)()
        S.raw("fl_ibm_force", h, ptr(S["F"]), ptr(S["dV"]), None, 1, about, force, torque)
        S.host("force", force[:]); S.host("torque", torque[:])
        S.release("u", "F", "dV")
    def created_set():                                          # both plays start from the set as it was created (fl_ibm_update waits: before the delay)
        with torch.cuda.stream(P.stream):
            capi.check(capi.lib.fl_ibm_update(h, ptr(first[0]), ptr(first[1]), ptr(first[2])), "fl_ibm_update")
    try:
        idle = both(f"{gname} IBM sequence", P, seq, inputs, outs, poison, before=created_set)
    finally:
        P.synchronize()
        capi.lib.fl_ibm_destroy(h)
        P.close()
    wX, wU, bX, bU = ir.rigid_pose(np.array(X0), c0, c, rotvec, vel, om)
    assert ir.rigid_pose_within(np.stack(idle["pose"][:3]), wX, bX) <= 1.0 and ir.rigid_pose_within(idle["pose"][3].reshape(3, L), wU, bU) <= 1.0
    Xn = [a.copy() for a in idle["pose"][:3]]
    assert np.allclose(idle["U1"][0].reshape(3, L), g.ibm_interp(kind, X0, u), rtol=1e-12, atol=1e-13)           # tests/test_gpu_ibm.py:67
    assert np.allclose(idle["U2"][0].reshape(3, L), g.ibm_interp(kind, Xn, u), rtol=1e-12, atol=1e-13)
    assert differ(idle["U1"][0], idle["U2"][0])


# ------------------------------------------------------------------------------------------------------------------ GMRES helpers

@TWO
def test_vec_maxpy_and_mdot_with_temporaries(pairs, gname):
    """the host array of k device pointers and the coefficients live in temporaries that are redirected (to a decoy array) / overwritten (NaN) and
    deleted as soon as the call has returned: fl_vec_maxpy only enqueues, so its launches must carry the values with them"""
    from fluca_amd import capi
    P, g, n, bc = pairs(gname)
    m, k = 3 * g.ncell, 11                                      # more vectors than one launch takes (8)
    rng = np.random.default_rng(404)
    x, Y, al = rng.standard_normal(m), rng.standard_normal((k, m)), rng.standard_normal(k)
    inputs = {"x": x, **{f"Y{j}": Y[j] for j in range(k)}}
    decoy = dev(rng.standard_normal(m))

    def seq(S):
        pa = (C.c_void_p * k)(*[S[f"Y{j}"].data_ptr() for j in range(k)])
        ca = (C.c_double * k)(*al)
        S.raw("fl_vec_maxpy", P.h, m, ptr(S["x"]), ca, pa, k)
        for j in range(k):
            pa[j], ca[j] = decoy.data_ptr(), NAN
        del pa, ca
        S.snap("maxpy", "x")
        S.still_pending(f"{gname} fl_vec_maxpy, k = {k}")
        pa = (C.c_void_p * k)(*[S[f"Y{j}"].data_ptr() for j in range(k)])
        out = (C.c_double * k)()
        S.raw("fl_vec_mdot", P.h, m, ptr(S["x"]), pa, k, out)
        for j in range(k):
            pa[j] = decoy.data_ptr()
        del pa
        S.host("mdot", out[:])
        S.release("x", *[f"Y{j}" for j in range(k)])
    idle = both(f"{gname} GMRES helpers", P, seq, inputs, {})
    xn = x + al @ Y
    assert np.allclose(idle["maxpy"][0], xn, rtol=1e-13, atol=1e-13)                                  # tests/test_gpu_momentum.py:502
    assert np.allclose(idle["mdot"][0], Y @ xn, rtol=1e-12, atol=1e-12)                               # :498


# ------------------------------------------------------------------------------------------------------------------ solves after queued work

def solve_seq(P, kw, second=True):
    """solve(b) with b's producer pending; then b <- 2 b - 0.5 x in place by an async call, and the solve again right behind it"""
    def seq(S):
        N = S["b"].numel()
        _, info = S.do(P.solve, S["b"], x=S["x"], history=kw.get("check_every", 0) >= 0, **kw)
        S.snap("x1", "x")
        S.host("stats1", [info["iters"], info["reason"]])
        if "history" in info:
            S.host("history1", info["history"])
        if second:
            S.raw("fl_vec_lincomb", P.h, N, 2.0, ptr(S["b"]), -0.5, ptr(S["x"]), ptr(S["b"]))
            _, info = S.do(P.solve, S["b"], x=S["x"], history=kw.get("check_every", 0) >= 0, **kw)
            S.snap("x2", "x")
            S.host("stats2", [info["iters"], info["reason"]])
            if "history" in info:
                S.host("history2", info["history"])
        S.release("b")
    return seq


@TWO
@pytest.mark.parametrize("solver", ["cg-jacobi", "chebyshev-fused"])
def test_poisson_solve_behind_a_pending_producer(pairs, gname, solver):
    P, g, n, bc = pairs(gname)
    ns = O not in bc
    S_ = g.assemble_S()
    b = mean_free_rhs(S_, g.ncell)[1] if ns else np.random.default_rng(5).standard_normal(g.ncell)
    if solver == "cg-jacobi":
        kw = dict(type=0, pc=fo.PC_JACOBI, norm_type=fo.NORM_PRECONDITIONED, remove_nullspace=int(ns), rtol=1e-5, maxit=10000, check_every=7)
    else:                                                       # exactly maxit steps, no poll, no statistics: the smoother's use
        lam = S_.gershgorin(fo.PC_JACOBI)
        kw = dict(type=2, pc=fo.PC_JACOBI, norm_type=fo.NORM_NONE, remove_nullspace=int(ns), maxit=12, emin=0.1 * lam, emax=1.1 * lam, check_every=-1)
    from fluca_amd import capi
    fuse = C.c_int()
    capi.check(capi.lib.fl_tuning_get(b"cheb_fuse", C.byref(fuse)))
    capi.check(capi.lib.fl_tuning_set(b"cheb_fuse", 2))         # two steps per sweep on every grid where that is legal: these grids are small
    try:
        idle = both(f"{gname} fl_poisson_solve {solver}", P, solve_seq(P, kw), {"b": b}, {"x": g.ncell}, must_assert=False)
    finally:
        capi.check(capi.lib.fl_tuning_set(b"cheb_fuse", fuse.value))
    if solver == "cg-jacobi":
        assert idle["stats1"][0][1] == 2 and idle["stats2"][0][1] == 2 and idle["stats1"][0][0] > 5
        x1 = idle["x1"][0]
        assert np.linalg.norm(b - S_.mult(x1)) <= 1e-3 * np.linalg.norm(b)
    assert differ(idle["x1"][0], idle["x2"][0])


def test_poisson_solve_multigrid_three_levels_behind_a_pending_producer():
    n, bc = (32, 32, 16), [V] * 6
    P, g = make_pair(n, bc, kappa=1e-3)
    try:
        S_ = g.assemble_S()
        p = np.random.default_rng(3).standard_normal(g.ncell)
        p -= p.mean()
        b = S_.mult(p)
        kw = dict(type=0, pc=2, remove_nullspace=1, rtol=1e-8, maxit=50, mg_levels=3)
        idle = both("(32, 32, 16) fl_poisson_solve CG + multigrid, 3 levels", P, solve_seq(P, kw), {"b": b}, {"x": g.ncell}, must_assert=False)
        assert idle["stats1"][0][1] == 2 and idle["stats2"][0][1] == 2
        x1 = idle["x1"][0]
        assert np.linalg.norm((x1 - x1.mean()) - p) <= 1e-6 * np.linalg.norm(p)                      # tests/test_gpu_mg.py:56-67
    finally:
        P.close()


@TWO
def test_momentum_solve_and_abf_apply_behind_a_pending_producer(pairs, gname):
    """fl_momentum_solve (BiCGStab) and fl_abf_apply with their right-hand sides still to be produced; x, iterations, reason and history against the
    idle bits"""
    from fluca_amd import capi
    from fluca_amd.poisson import KspOptions, Momentum
    P, g, n, bc = pairs(gname)
    ns = O not in bc
    M = Momentum(P)
    N, nf = g.ncell, [int(a) for a in g.nface]
    rng = np.random.default_rng(31)
    V0 = [rng.standard_normal(nf[d]) for d in range(3)]
    W = [rng.standard_normal(nf[q % 3]) for q in range(9)]
    rho, mu = 1.0, 0.5 * min(np.diff(g.xf[d]).min() for d in range(3))
    dt = g.kappa * rho
    keep = [[dev(a) for a in V0], [dev(a) for a in W]]
    M.set_state(dt, rho, mu, keep[0], keep[1])
    M.set_ainv_types(schur=fo.AINV_ID, upper=fo.AINV_ID)
    momrhs = rng.standard_normal(3 * N)
    ir_ = [1e-2 * rng.standard_normal(nf[d]) for d in range(3)]
    if ns:                                                      # no flux through the walls (tests/test_gpu_caller_arrays.py::test_abf_apply)
        for d in range(3):
            if bc[2 * d] != PER:
                shp = [n[2], n[1], n[0]]
                shp[2 - d] = nf[d] // (N // n[d])
                a = ir_[d].reshape(shp)
                sl = [slice(None)] * 3
                for side in (0, -1):
                    sl[2 - d] = side
                    a[tuple(sl)] = 0.0
    mo = KspOptions(type=capi.KSP_BCGS, rtol=1e-10, maxit=500)
    so_ = KspOptions(rtol=1e-10, maxit=5000, remove_nullspace=int(ns))
    inputs = {"momrhs": momrhs, **{f"ir{d}": ir_[d] for d in range(3)}}
    outs = {"xs": 3 * N, "v": 3 * N, "p": N, **{f"V{d}": nf[d] for d in range(3)}}

    def seq(S):
        _, info = S.do(M.solve, S["momrhs"], x=S["xs"], history=True, pc=fo.PC_JACOBI, rtol=1e-8, maxit=500)
        S.snap("xs", "xs")
        S.host("mom", [info["iters"], info["reason"]]); S.host("mom_history", info["history"])
        st = (capi.fl_ksp_stats * 2)()
        S.raw("fl_abf_apply", M.h, C.byref(mo.o), C.byref(so_.o), ptr(S["momrhs"]), ptrs([S[f"ir{d}"] for d in range(3)]), None, ptr(S["v"]),
              ptrs([S[f"V{d}"] for d in range(3)]), ptr(S["p"]), st)
        S.snap("abf", ["v", "p", "V0", "V1", "V2"])
        S.host("abf_stats", [st[0].iters, st[0].reason, st[1].iters, st[1].reason])
        S.release("momrhs", "ir0", "ir1", "ir2")
    try:
        idle = both(f"{gname} fl_momentum_solve + fl_abf_apply", P, seq, inputs, outs, must_assert=False)
    finally:
        M.close()
    A = g.assemble_momentum(1.0, dt, -0.5 * mu * dt / rho, V0, W)
    assert idle["mom"][0][1] > 0 and np.linalg.norm(momrhs - A.mult(idle["xs"][0])) <= 50 * 1e-8 * np.linalg.norm(momrhs)      # tests/test_gpu_momentum.py:94-102
    assert idle["abf_stats"][0][1] > 0 and idle["abf_stats"][0][3] > 0


# ------------------------------------------------------------------------------------------------------------------ two ranks in one process

def _two_rank_worker(R, case, blocks):
    """rank 0 queues the delay and its pending producers; rank 1 runs ahead.  fl_poisson_apply (halo exchange through comm_stream) and fl_scalar_rhs"""
    from fluca_amd.scalar import Scalar
    from tests.test_gpu_config5 import _handle
    P, d, s = _handle(R, case)
    with torch.cuda.stream(s):
        Sc = Scalar(P, case.kinds, case.vals, limiter="superbee", gamma=GAMMA)
        Vb = [np.ascontiguousarray(blocks["V"][a][R.rank]).ravel() for a in range(3)]
        phi, q, x = blocks["phi"][R.rank].ravel(), blocks["q"][R.rank].ravel(), blocks["x"][R.rank].ravel()
        N = phi.size
        inputs = {"x": x, "phi": phi, "q": q, **{f"V{a}": Vb[a] for a in range(3)}}

        def seq(S):
            S.do(P.apply, S["x"], S["y"]); S.snap("apply", "y")
            Sc.set_velocity(S["V0"], S["V1"], S["V2"])
            S.do(Sc.rhs, S["phi"], S["q"], out=S["R"]); S.snap("rhs", "R")
            S.release("x", "phi", "q", "V0", "V1", "V2")
        idle = both(f"(1, 1, 2) rank {R.rank} fl_poisson_apply + fl_scalar_rhs", P, seq, inputs, {"y": N, "R": N}, delay=R.rank == 0, must_assert=False)
        Sc.close()
    P.close()
    return {k: v[0] for k, v in idle.items()}


def test_two_ranks_one_delayed():
    """G2 on a (1, 1, 2) rank grid in this process (tests/inproc.py).  No ghost layer may be packed from an array whose producer is still pending: each
    rank's queued bits equal its idle bits, and the gathered idle results are the undecomposed operator's."""
    from tests import scalar_reference as sref
    n = GRIDS["G2"][0]
    case = rk.Case(n, (1, 1, 2), "neumann", uniform=True)
    Vv = sc.velocity(n, "neumann")
    phi, q = sc.phi_field(n, "random"), sc.source(n)
    x = np.random.default_rng(7).standard_normal(phi.shape)
    blocks = {"V": [rk.scatter_faces(case, Vv[a], a) for a in range(3)], "q": rk.scatter_cells(case, q), "phi": rk.scatter_cells(case, phi), "x": rk.scatter_cells(case, x)}
    res = inproc.run_threads(case.size, _two_rank_worker, case, blocks)
    kinds, vals = sc.BC_SETS["neumann"]
    Pr = sref.Problem(sc.faces(n, True), kinds, vals, GAMMA, "superbee")
    want, E, _ = sref.rhs(Pr, phi, Vv, q, np.longdouble, bounds=True, limiter="superbee")
    got = rk.gather_cells(case, [res[r]["rhs"] for r in range(case.size)])
    err = np.abs(got.astype(np.longdouble) - want).astype(np.float64)
    assert (err <= sc.rhs_slack(E)).all(), float((err / sc.rhs_slack(E)).max())
    g = fo.Grid(n, sc.faces(n, True), sc.poisson_bc(kinds), 1e-3)
    S_ = g.assemble_S()
    y = rk.gather_cells(case, [res[r]["apply"] for r in range(case.size)]).ravel()
    ref = S_.mult(x.ravel())
    assert abs(y - ref).max() <= 1e-13 * abs(S_.arrays()[2]).max() * 7 * abs(x).max()
