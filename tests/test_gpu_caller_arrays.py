"""-m gpu: the entry points of the C-ABI that read or write a caller's array (listed below), on arrays a foreign caller hands in: views into ONE allocation
(tests/caller_arrays.py) that are 8 bytes off a 16-byte boundary, or packed back to back as the blocks of a nest vector are, with guard words
around them.  Every other GPU test hands the library arrays that are each their own torch allocation: 256-byte aligned and followed by slack.

What the host decides from a pointer's low bits (all of it): launch_project_all and project_six_usable (fl_kernels.hip, with
fl_poisson_project), unpadded_pairs (k_cg_init reading b, k_cg_finish writing x), mom_apply_t (k_mom2 / k_mom3 storing y), mom_pw (k_mom_pw3
reading b) and the buoyancy kernel's mask (tests/test_gpu_buoyancy.py).  Each takes its 16-byte branch for an aligned base AND an even nx.

Every case runs on arrays of their own (the ordinary call), then PENDING (below), then in placement A (the control: aligned, guarded), then B (8 bytes
off), D (packed) and, where named, C (alternating), and asserts:
  1. Arena.check: no guard word, no input and no array the call may not write changed by a bit; every output entry lost its sentinel;
  2. every result is finite;
  3. the result against the reference and at the tolerance of the entry point's own test (named beside each check) -- no tolerance is new here;
  4. placement A gives the ordinary call's bits;
  5. every placement gives placement A's bits: the branches of a dispatch differ in access width only, and no lane-to-element map depends on the
     base.  The Krylov solves are held to this as well as to their references: only their first and last kernels touch the caller's arrays, with
     the same arithmetic per entry in both branches, and a reference's tolerance (50 rtol) would let a wrong entry of the 8-byte branch pass;
  6. fl_poisson_project took the route the placement calls for (fldbg_project_path); for the two-way dispatches the phase the arena asserted
     together with the parity of nx names the branch, and each run prints both.

  7. the PENDING run (drive): the same call on the same handle behind a delay queued on the handle's stream (tests/stream_order.py: DELAY_MS of
     torch.cuda._sleep, no host callback), its inputs still poison when the call is made -- their producer, a device-to-device copy, is queued on the
     stream behind the delay -- and poisoned again in stream order right after; arrays the header calls copied are poisoned as soon as they are
     handed over (T.release), borrowed ones after the last call that reads them.  Poison is NaN; marker positions, which become cell indices, are
     another valid marker set instead.  Every result is finite and has the ordinary run's bits, and where every entry point of the case is `async`
     in tests/stream_order.py the delay had not ended when call(T) returned: the host did not wait.  Each run prints the host time of call(T).

Grids: the smallest at which each branch is live (GRIDS below), at most 3510 cells.  IBM runs on the same shapes with walls and, on G4, its
periodic x (the kernels know walls and periodic axes, and a periodic axis needs twice the support in cells: fl_ibm_create), the scalar on the same shapes
with the boundary set of tests/scalar_cases.py that has the same periodic axes.  G1 and G5 have one multigrid level: CG + multigrid runs there
as tests/test_gpu_mg.py::test_one_level_hierarchy_keeps_the_outer_residual holds it.

Covered: fl_poisson_apply, _diagonal, _rhs, _project, _gst_bc, _solve (five solvers); fl_boundary_set_faces, _add_faces, _add_cells;
fl_pressure_update; fl_momentum_set_state, _set_state_v0, _apply, _diagonal, _rowsum, _solve (four), _face_interp, _face_interp_scaled,
_interp_faces, _interp_faces_ends, _rhs, _add_buoyancy; fl_abf_jacobian_mult, _apply, _schur_apply; fl_vec_lincomb, _dot, _mdot, _maxpy;
fl_layout_{from,to}_dmstag_{local,global}; fl_ibm_create, _update, _interp, _spread, _force (one body), _rigid_pose; fl_scalar_set_velocity, _rhs,
_step, _stats, _cfl, _boundary_flux.
NOT covered, and so not held to the contract by this file: the int32 body ids of fl_ibm_force and the owner-rank marker calls
fl_ibm_owned_select, fl_ibm_create_owned, fl_ibm_migrate, fl_ibm_owned_fetch.  The ids and the owner-rank calls' index arrays are integers,
which the fp64 arena does not hold; their own tests use arrays of their own.  The owner-rank calls are collective and wait by design: they are
not run pending either (tests/stream_order.py).  Sequences of calls queued behind ONE delay: tests/test_gpu_stream_order.py."""
import ctypes as C
import math
import time

import numpy as np
import pytest
import torch

from oracle import fluca_oracle as fo
from tests import inproc
from tests import scalar_cases as sc
from tests import scalar_ranks as rk
from tests import scalar_reference as sref
from tests import step_rhs as sr
from tests import stream_order as so
from tests.caller_arrays import SENTINEL, SENTINEL_BITS, Arena
from tests.gpu_common import CAVITY, CAVITY_BOX, O, PER, V, dev, make_pair, mean_free_rhs

pytestmark = pytest.mark.gpu

GRIDS = {
    "G1": ((6, 5, 4), [V] * 6),                    # even nx, ny <= 8 (k_mom2), one partial segment
    "G2": ((12, 9, 5), CAVITY),                    # even nx; 13 * 9 * 5 = 585 x-faces: packed [Vx | Vy | Vz] shifts Vy and Vz; ny > 8 (k_mom3)
    "G3": ((130, 9, 3), [V, O, V, V, PER, PER]),   # a second 128-cell segment with a two-cell tail, outlet rows, fz = nz
    "G4": ((128, 4, 3), [PER] * 6),                # a full segment, fx = nx, wrapped taps of k_project_six on the caller's p, ny < 8 (one slab)
    "G5": ((7, 5, 3), [V] * 6),                    # odd nx (no pairs anywhere), odd N = 105: component d of a 3 N array alternates phase even in A
}
SCALAR_BC = {"G1": "dirichlet", "G2": "neumann", "G3": "channel", "G4": "periodic", "G5": "dirichlet"}      # the same periodic axes
ABD, ABCD = ("A", "B", "D"), ("A", "B", "C", "D")
SIX_DIRECT, SIX_PADDED, ALL_PAIRS, ALL_SINGLE = range(4)            # fldbg_project_path
PATH_NAME = ["k_project_six on the caller's p", "k_project_six on the padded p", "k_project_all with pairs", "k_project_all without pairs"]


# ------------------------------------------------------------------------------------------------------------------ the driver

def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def ptrs(ts):
    return (C.c_void_p * len(ts))(*[None if t is None else t.data_ptr() for t in ts])


def quiet(call):
    """a call whose return value (the output tensor) is not a further result"""
    def f(T):
        call(T)
    return f


def raw(P, fn, *args):
    """a C-ABI call on the handle's stream, ordered against torch's"""
    from fluca_amd import capi
    P._pre()
    rc = getattr(capi.lib, fn)(*args)
    P._post()
    assert rc == 0, (fn, rc)


class Ordinary:
    """the interface of an Arena on arrays that are each their own allocation"""
    placement = "ordinary"

    def __init__(self, spec, inputs):
        self.t = {n: (torch.full((l,), SENTINEL, dtype=torch.float64, device="cuda") if r == "out" else _dev(inputs[n])) for n, l, r in spec}

    def __getitem__(self, name):
        return self.t[name]

    def phase(self, name):
        return self.t[name].data_ptr() % 16

    def get(self, name):
        return self.t[name].cpu().numpy().copy()


def _dev(a):
    return torch.from_numpy(np.array(a, dtype=np.float64).reshape(-1)).to("cuda")


class Pending(Ordinary):
    """arrays of their own whose inputs are still to be PRODUCED when the call is made: every "in" / "inout" array starts as poison (NaN, or the valid
    other input the case names for what becomes an index or a branch), produce() copies the true inputs in through staging tensors on the device -- in
    stream order, behind the delay --, release(names) puts the poison back in stream order (the caller reuses its buffers), snapshot() clones the
    results in stream order"""
    placement = "pending"

    def __init__(self, spec, inputs, poison):
        self.spec = spec
        self.src = {n: _dev(inputs[n]) for n, l, r in spec if r != "out"}
        self.poison = {n: (_dev(poison[n]) if n in poison else torch.full((l,), float("nan"), dtype=torch.float64, device="cuda")) for n, l, r in spec if r != "out"}
        for n, l, r in spec:
            assert r == "out" or (self.poison[n].numel() == l and not torch.equal(self.poison[n], self.src[n]) or l == 0), (n, "the poison must differ from the input")
        self.stage = {n: p.clone() for n, p in self.poison.items()}         # the staging tensors are themselves complete only behind the delay
        self.t = {n: (torch.full((l,), SENTINEL, dtype=torch.float64, device="cuda") if r == "out" else self.poison[n].clone()) for n, l, r in spec}
        self.snap = {}

    def fill_staging(self):
        for n, src in self.src.items():
            self.stage[n].copy_(src)

    def produce(self):
        """the producer: the arrays from the staging tensors, which fill_staging() completed earlier on the SAME stream -- a producer that ran anywhere
        else would hand on the staging tensors' poison"""
        for n in self.src:
            self.t[n].copy_(self.stage[n])

    def release(self, *names):
        for n in names:
            self.t[n].copy_(self.poison[n])

    def snapshot(self, names):
        self.snap = {n: self.t[n].clone() for n in names}

    def get(self, name):
        return self.snap[name].cpu().numpy().copy()


def drive(label, spec, inputs, call, written, placements=ABD, partial=(), flips=(), verify=None, nx=None, P=None, fns=(), poison=None, ranks=False):
    """call(T) on the ordinary arrays, PENDING (below) and in every placement (flips: further runs in A with these arrays 8 bytes off); T[name] is
    the array.  call returns further host results or None.  -> the results of every run, by run name.
    P, fns: the handle whose stream the calls run on and the entry points call(T) makes (rows of tests/stream_order.py).  The pending run, on the same
    handle right after the ordinary one (first-use allocations and tables exist): everything under torch.cuda.stream(P.stream); on that stream a
    delay, an event, the copies that complete the staging tensors, the producer of every input (array <- staging tensor), then call(T); the moment it returns, has the delay ended? (it must not have where all of fns are
    `async`: else the entry point waited, or the run proved nothing); then, in stream order, the results are cloned and every "in" array is poisoned
    again.  A case that hands an array over and uses the handle later calls T.release(names) between the two (a no-op in every other run).  The
    results must be finite and have the ordinary run's bits (tests/test_gpu_handle_history.py: a repeat on one handle is bitwise the same).
    ranks: one rank of several -- the peers and a host-staged transport make a call wait, so the delay is not asserted."""
    for n, l, r in spec:
        assert r == "out" or np.asarray(inputs[n]).size == l, (label, n)
    assert P is not None and fns and all(f in so.TABLE for f in fns), (label, fns)
    runs = [("ordinary", ()), ("pending", ())] + [(p, ()) for p in placements] + [("A", tuple(f)) for f in flips]
    out, base = {}, None
    for placement, flip in runs:
        if placement == "ordinary":
            T = Ordinary(spec, inputs)
        elif placement == "pending":
            T = Pending(spec, inputs, poison or {})
        else:
            T = Arena(spec, placement, "cuda", flip=flip)
            for n, l, r in spec:
                if r != "out":
                    T.fill(n, inputs[n])
            T.freeze()
        tag = T.tag = placement + ("".join("+" + f for f in flip))
        ph = {n: T.phase(n) for n, _, _ in spec}
        pairs = "" if nx is None else f", nx {'even' if nx % 2 == 0 else 'odd'}: 16-byte branch for {[n for n in ph if nx % 2 == 0 and ph[n] == 0]}"
        print(f"{label} [{tag}] phases {ph}{pairs}")
        kind = "async" if so.all_async(fns) and not ranks else "waits"
        if placement == "pending":
            torch.cuda.synchronize()
            with torch.cuda.stream(P.stream):               # the handle's own stream is the current one: _pre / _post order it against itself
                e_delay = so.Delay.queue()
                T.fill_staging()
                T.produce()
                t0 = time.perf_counter()
                extra = call(T) or {}
                ended = e_delay.query()
                ms = (time.perf_counter() - t0) * 1e3
                T.snapshot(written)
                T.release(*[n for n, _, r in spec if r == "in"])
            P.stream.synchronize()
            print(f"{label} [{tag}] class {kind}: host time of call(T) {ms:.3f} ms, the delay had {'ENDED' if ended else 'not ended'} when it returned"
                  + ("" if kind == "async" else " (not asserted)"))
            assert kind != "async" or not ended, (label, fns, f"call(T) took {ms:.3f} ms on the host and returned after the {so.DELAY_MS} ms delay: an async entry point waited")
        else:
            if not hasattr(T, "release"):
                T.release = lambda *names: None
            t0 = time.perf_counter()
            extra = call(T) or {}
            print(f"{label} [{tag}] class {kind}: host time of call(T) {(time.perf_counter() - t0) * 1e3:.3f} ms")
        if placement not in ("ordinary", "pending"):
            T.check(written=written, partial=partial)
        res = {n: T.get(n) for n in written}
        res.update(extra)
        for k, v in res.items():
            assert np.isfinite(np.asarray(v, dtype=np.float64)).all(), (label, tag, k, "not finite")
        if placement == "ordinary":
            assert all(p == 0 for p in ph.values()), "an allocation of its own is 16-byte aligned"
            for n in written:                                   # what the arena asserts of an output, for the ordinary arrays
                if dict((a, c) for a, _, c in spec)[n] == "out" and n not in partial:
                    assert not (bits(res[n]) == SENTINEL_BITS).any(), (label, n, "an output entry was not written")
            base = res
        if placement != "ordinary":
            assert sorted(res) == sorted(base), (label, tag)
            differ = [k for k in base if not same_bits(res[k], base[k])]
            print(f"{label} [{tag}] the ordinary call's bits: {not differ}")
            assert not differ, (label, tag, differ, "differs from the ordinary call and placement A by bits", _first_diff(res[differ[0]], base[differ[0]]))
        if verify is not None:
            verify(res, f"{label} [{tag}]")
        out[tag] = res
    return out


def _first_diff(a, b):
    a, b = np.asarray(a, dtype=np.float64).ravel(), np.asarray(b, dtype=np.float64).ravel()
    bad = np.flatnonzero(bits(a) != bits(b))
    return (int(bad.size), int(bad[0]), float(a[bad[0]]), float(b[bad[0]])) if bad.size else None


# ------------------------------------------------------------------------------------------------------------------ grids and handles

class Ctx:
    def __init__(self, name):
        self.name = name
        self.n, self.bc = GRIDS[name]
        self.P, self.g = make_pair(self.n, self.bc, kappa=1e-3)
        self.N, self.nface = self.g.ncell, tuple(self.g.nface)
        assert self.P.ncell == self.N and tuple(self.P.nface) == self.nface
        self.nullspace = O not in self.bc
        self.rng = np.random.default_rng(20261019 + int(name[1]))
        self._S = self._M = self._state = self._abf = None
        self.keep = []

    @property
    def S(self):
        if self._S is None:
            self._S = self.g.assemble_S()
        return self._S

    def b(self):
        """the right-hand side of tests/test_gpu_poisson.py: S p* with a mean-free p* where S has a null space, else random"""
        return mean_free_rhs(self.S, self.N)[1] if self.nullspace else np.random.default_rng(5).standard_normal(self.N)

    @property
    def M(self):
        if self._M is None:
            from fluca_amd.poisson import Momentum
            self._M = Momentum(self.P)
        return self._M

    def cheb_state(self):
        """the state of tests/test_gpu_momentum_cheb.py (CFL-sized convection beside a viscous part of the same size), handed over with v0: k_mom3
        where ny > 8, k_mom2 elsewhere.  -> the assembled A"""
        from tests.test_gpu_momentum_cheb import _state
        g, M = self.g, self.M
        if self._state is None:
            V0, v0, dt, rho, mu = _state(g, 0.4)
            W = g.apply_B(v0)
            self._state = (V0, v0, dt, rho, mu, g.assemble_momentum(1.0, dt, -0.5 * mu * dt / rho, V0, W))
        V0, v0, dt, rho, mu, A = self._state
        self.keep = [[dev(a) for a in V0], M.interp_faces(dev(v0)), dev(v0)]
        M.set_state(dt, rho, mu, self.keep[0], self.keep[1], v0=self.keep[2])
        M.set_ainv_types(schur=fo.AINV_ID, upper=fo.AINV_ID)
        return A

    def abf_state(self):
        """the state of tests/test_gpu_momentum.py::_state: dt of the pair's kappa, a noticeably non-unit diagonal.  -> (A, dt, rho, mu)"""
        g, M = self.g, self.M
        mu, scale = 0.05, 8.0
        if self._abf is None:
            rng = np.random.default_rng(3)
            V0 = [scale * rng.standard_normal(g.nface[d]) for d in range(3)]
            W = [scale * rng.standard_normal(g.nface[d]) for c in range(3) for d in range(3)]
            rho = 1.0
            dt = g.kappa * rho
            self._abf = (V0, W, dt, rho, g.assemble_momentum(1.0, dt, -0.5 * mu * dt / rho, V0, W))
        V0, W, dt, rho, A = self._abf
        self.keep = [[dev(a) for a in V0], [dev(a) for a in W]]
        M.set_state(dt, rho, mu, self.keep[0], self.keep[1])
        return A, dt, rho, mu

    def close(self):
        if self._M is not None:
            self._M.close()
        self.P.close()


@pytest.fixture(scope="module")
def ctx():
    made = {}

    def get(name):
        if name not in made:
            made[name] = Ctx(name)
        return made[name]
    yield get
    for c in made.values():
        c.close()


GN = pytest.mark.parametrize("gname", list(GRIDS))


def close(got, want, tol=2e-13):
    """_close of tests/test_gpu_momentum.py:41-43"""
    scale = np.abs(want).max()
    assert np.abs(got - want).max() <= tol * scale, (np.abs(got - want).max(), scale)


# ------------------------------------------------------------------------------------------------------------------ the Poisson operator

@GN
def test_apply_and_diagonal(ctx, gname):
    c = ctx(gname)
    P, S, N = c.P, c.S, c.N
    x = np.random.default_rng(7).standard_normal(N)
    ref = S.mult(x)
    scale = abs(S.arrays()[2]).max() * 7 * abs(x).max()

    def verify(res, what):                                      # tests/test_gpu_poisson.py:39-41
        assert abs(res["y"] - ref).max() <= 1e-13 * scale, what
    drive(f"{gname} fl_poisson_apply", [("x", N, "in"), ("y", N, "out")], {"x": x}, quiet(lambda T: P.apply(T["x"], T["y"])), ["y"], verify=verify, nx=c.n[0],
          P=P, fns=["fl_poisson_apply"])

    def verify_d(res, what):                                    # tests/test_gpu_poisson.py:43
        assert np.allclose(res["d"], S.diag(), rtol=1e-14, atol=0), what
    drive(f"{gname} fl_poisson_diagonal", [("d", N, "out")], {}, lambda T: raw(P, "fl_poisson_diagonal", P.h, ptr(T["d"])), ["d"], verify=verify_d, nx=c.n[0], P=P, fns=["fl_poisson_diagonal"])


@GN
@pytest.mark.parametrize("with_contrhs", [True, False], ids=["contrhs", "no-contrhs"])
def test_rhs(ctx, gname, with_contrhs):
    c = ctx(gname)
    P, g, N = c.P, c.g, c.N
    rng = np.random.default_rng(3)
    Vf = [rng.standard_normal(nf) for nf in g.nface]
    cr = rng.standard_normal(N)
    ref = g.rhs(*Vf, contrhs=cr if with_contrhs else None)
    bound = 1e-12 * max(1.0, abs(g.rhs(*Vf, contrhs=cr)).max())      # tests/test_gpu_poisson.py:56-58
    spec = [("Vx", g.nface[0], "in"), ("Vy", g.nface[1], "in"), ("Vz", g.nface[2], "in"), ("contrhs", N, "in"), ("b", N, "out")]

    def call(T):
        P.rhs(T["Vx"], T["Vy"], T["Vz"], contrhs=T["contrhs"] if with_contrhs else None, b=T["b"])

    def verify(res, what):
        assert abs(res["b"] - ref).max() <= bound, what
    drive(f"{gname} fl_poisson_rhs", spec, dict(Vx=Vf[0], Vy=Vf[1], Vz=Vf[2], contrhs=cr), call, ["b"], verify=verify, nx=c.n[0], P=P, fns=["fl_poisson_rhs"])


# ------------------------------------------------------------------------------------------------------------------ the projection

PROJ = ["p", "v0", "v1", "v2", "V0", "V1", "V2"]


def project_path(P, T, use):
    from fluca_amd import capi
    f = capi.lib.fldbg_project_path
    f.restype = C.c_int
    f.argtypes = [C.c_void_p] * 8 + [C.POINTER(C.c_int)]
    out = C.c_int(-1)
    assert f(P.h, ptr(T["p"]), *[ptr(T[n]) if n in use else None for n in PROJ[1:]], C.byref(out)) == 0
    return out.value


def expected_path(nx, several, phase, use):
    """the rule of fl_poisson_project (fl_api.hip) restated from the phases: V0's rows are nx + 1 long, so its base does not count"""
    counted = [n for n in PROJ[1:] if n in use and n != "V0"]
    aligned = nx % 2 == 0 and all(phase[n] == 0 for n in counted)
    if aligned and len(use) == 6:
        return SIX_DIRECT if (not several and phase["p"] == 0) else SIX_PADDED
    return ALL_PAIRS if aligned else ALL_SINGLE


def project_arrays(p, vs, Vf):
    """all seven arrays stand in the arena whichever of them a call names: the others must not change"""
    N = p.size
    spec = [("p", N, "in")] + [(f"v{d}", N, "inout") for d in range(3)] + [(f"V{d}", Vf[d].size, "inout") for d in range(3)]
    inputs = {"p": p, **{f"v{d}": vs[d] for d in range(3)}, **{f"V{d}": Vf[d] for d in range(3)}}
    return spec, inputs


def run_project(label, P, nx, spec, inputs, use, placements, flips, several, want, seen):
    """the projection of the arrays named in `use`; seen collects the routes taken.  -> the results of every run"""
    def call(T):
        phase = {n: T.phase(n) for n in PROJ}
        path = project_path(P, T, use)
        print(f"{label} [{T.tag}] fldbg_project_path -> {path} ({PATH_NAME[path]})")
        assert path == expected_path(nx, several, phase, use), (label, T.placement, path, phase)
        if all(ph == 0 for ph in phase.values()) and nx % 2 == 0:      # ordinary arrays, placement A
            assert path == ((SIX_PADDED if several else SIX_DIRECT) if len(use) == 6 else ALL_PAIRS)
        if (T.placement == "B" and all(phase[n] == 8 for n in use)) or nx % 2:
            assert path == ALL_SINGLE
        seen.setdefault(path, []).append((label, T.tag))
        P.project(T["p"], v=[T[f"v{d}"] if f"v{d}" in use else None for d in range(3)], V=[T[f"V{d}"] if f"V{d}" in use else None for d in range(3)])

    def verify(res, what):                                      # tests/test_gpu_poisson.py:66-73
        for n in use:
            assert abs(res[n] - want[n]).max() <= 1e-12 * max(1.0, abs(want[n]).max()), (what, n)
    return drive(label, spec, inputs, call, sorted(use), placements=placements, flips=flips, verify=verify, nx=nx, P=P, fns=["fl_poisson_project"], ranks=several)


def project_fields(g, seed=11):
    rng = np.random.default_rng(seed)
    p = rng.standard_normal(g.ncell)
    Vf = [rng.standard_normal(nf) for nf in g.nface]
    vs = [rng.standard_normal(g.ncell) for _ in range(3)]
    Gst, Gc = g.apply_gst(p), g.apply_G(p)
    want = {**{f"V{d}": Vf[d] - Gst[d] for d in range(3)}, **{f"v{d}": vs[d] - Gc[d] for d in range(3)}}
    return p, vs, Vf, want


@GN
def test_project(ctx, gname):
    """all six arrays in A, B, C, D and with only p misaligned; the subset v = (v0, -, -), V = (-, V1, -) in A, B, C, D.  On G1 - G4 the four routes of
    fl_poisson_project all occur: six-direct (A), six on the padded p (only p misaligned), k_project_all with pairs (the subset in A) and without (B);
    the subset gives the bits of the six-array call (tests/test_gpu_poisson.py::test_projection_of_all_six_arrays)."""
    c = ctx(gname)
    P, g, nx = c.P, c.g, c.n[0]
    p, vs, Vf, want = project_fields(g)
    spec, inputs = project_arrays(p, vs, Vf)
    seen = {}
    six = run_project(f"{gname} fl_poisson_project six", P, nx, spec, inputs, set(PROJ[1:]), ABCD, [("p",)], False, want, seen)
    sub = run_project(f"{gname} fl_poisson_project subset", P, nx, spec, inputs, {"v0", "V1"}, ABCD, [("v0",), ("V1",), ("V0",)], False, want, seen)
    for tag, res in sub.items():
        for n in ("v0", "V1"):
            assert same_bits(res[n], six["A"][n]), (tag, n)
    if nx % 2 == 0:
        assert sorted(seen) == [SIX_DIRECT, SIX_PADDED, ALL_PAIRS, ALL_SINGLE], seen
    else:
        assert sorted(seen) == [ALL_SINGLE], seen


# ------------------------------------------------------------------------------------------------------------------ boundary vectors, pressure

def layer(shape, ax, side):
    sl = [slice(None)] * 3
    sl[2 - ax] = -1 if side else 0
    return tuple(sl)


@GN
@pytest.mark.parametrize("b", [1, 2, 5])
def test_boundary_kernels(ctx, gname, b):
    """fl_boundary_set_faces / add_faces / add_cells and fl_poisson_gst_bc on the high x, low y and high z boundary: the layer as
    tests/test_gpu_step_rhs.py:231-237, 243-251 hold it (set and the outlet vector bit for bit, add to one unit in the last place), every other
    entry of the target unchanged; nothing at all where the axis is periodic or the boundary no outlet"""
    c = ctx(gname)
    P, g, n = c.P, c.g, c.n
    ax, side = b // 2, b % 2
    shp_c = (n[2], n[1], n[0])
    nf = [int(g.nface[d]) // (c.N // n[d]) for d in range(3)]
    shp_f = tuple(nf[ax] if 2 - ax == i else s for i, s in enumerate(shp_c))
    pshape = tuple(s for i, s in enumerate(shp_c) if i != 2 - ax)
    rng = np.random.default_rng(40 + b)
    plane = rng.standard_normal(pshape)
    coeff = -1.37
    periodic = c.bc[b] == PER
    for fn, shp in (("fl_boundary_set_faces", shp_f), ("fl_boundary_add_faces", shp_f), ("fl_boundary_add_cells", shp_c), ("fl_poisson_gst_bc", shp_f)):
        before = rng.standard_normal(shp)
        m = before.size
        lay = layer(shp, ax, side)
        gst = fn == "fl_poisson_gst_bc"
        nothing = periodic or (gst and c.bc[b] != O)

        def call(T):
            if gst:
                raw(P, fn, P.h, b, ptr(T["plane"]), ptr(T["target"]))
            else:
                raw(P, fn, P.h, b, coeff, ptr(T["plane"]), ptr(T["target"]))

        def verify(res, what):
            after = res["target"].reshape(shp)
            if nothing:
                assert same_bits(after, before), what
                return
            if fn == "fl_boundary_set_faces":
                assert same_bits(after[lay], coeff * plane), what
            elif gst:                                           # tests/test_gpu_poisson.py:320
                assert np.allclose(after[lay], g.gst_bc_coeff(ax, side) * plane, rtol=1e-15, atol=0), what
            else:
                sr.one_ulp_of_any(after[lay], [before[lay] + coeff * plane, sr.fused(coeff, plane, before[lay])], what)
            rest = after.copy()
            rest[lay] = before[lay]
            assert same_bits(rest, before), what + " wrote outside its layer"
        drive(f"{gname} {fn} boundary {b}", [("plane", plane.size, "in"), ("target", m, "inout")], {"plane": plane, "target": before}, call,
              ["target"], verify=verify, nx=n[0], P=P, fns=[fn])


@GN
def test_pressure_update(ctx, gname):
    """first step (p = p0 + 2 dp, phalf = p0 + dp: single roundings, bit for bit) and a later one (p = phalf + 1.5 dp fused or not, phalf += dp):
    tests/test_gpu_step_rhs.py:439-446"""
    c = ctx(gname)
    P, N = c.P, c.N
    rng = np.random.default_rng(5)
    dp, p0, ph = rng.standard_normal(N), rng.standard_normal(N), rng.standard_normal(N)

    def verify_first(res, what):
        assert same_bits(res["p"], 2.0 * dp + p0) and same_bits(res["phalf"], dp + p0), what
    drive(f"{gname} fl_pressure_update first", [("dp", N, "in"), ("p0", N, "in"), ("phalf", N, "out"), ("p", N, "out")], dict(dp=dp, p0=p0),
          lambda T: P.pressure_update(True, T["dp"], T["p0"], T["phalf"], T["p"]), ["phalf", "p"], verify=verify_first, nx=c.n[0], P=P, fns=["fl_pressure_update"])

    def verify_later(res, what):
        sr.one_ulp_of_any(res["p"], [1.5 * dp + ph, sr.fused(1.5, dp, ph)], what)
        assert same_bits(res["phalf"], ph + dp), what
    drive(f"{gname} fl_pressure_update later", [("dp", N, "in"), ("phalf", N, "inout"), ("p", N, "out")], dict(dp=dp, phalf=ph),
          lambda T: P.pressure_update(False, T["dp"], None, T["phalf"], T["p"]), ["phalf", "p"], verify=verify_later, nx=c.n[0], P=P, fns=["fl_pressure_update"])


# ------------------------------------------------------------------------------------------------------------------ the Schur solves

def solve_extras(info):
    out = dict(iters=info["iters"], reason=info["reason"], rnorm=info["rnorm"], rnorm0=info["rnorm0"])
    if "history" in info:
        out["history"] = info["history"]
    return out


def check_cg(c, b, xo, io, res, rtol, what):
    """_check_solve of tests/test_gpu_poisson.py:117-138"""
    S, xg = c.S, res["x"]
    assert res["reason"] == io["reason"], (what, res["reason"], io["reason"])
    assert abs(res["iters"] - io["iters"]) <= 2, (what, res["iters"], io["iters"])
    m = min(len(res["history"]), len(io["history"]))
    ho, hg = io["history"][:m], res["history"][:m]
    assert np.allclose(hg[: min(m, 5)], ho[: min(m, 5)], rtol=1e-9, atol=0), what
    assert np.allclose(hg, ho, rtol=1e-6, atol=1e-300), what
    bn = np.linalg.norm(b)
    assert np.linalg.norm(b - S.mult(xg)) <= 1.5 * np.linalg.norm(b - S.mult(xo)) + 1e-12 * bn, what
    if c.nullspace:
        xg, xo = xg - xg.mean(), xo - xo.mean()
    assert np.linalg.norm(xg - xo) <= 50 * rtol * np.linalg.norm(xo) + 1e-14, what


SOLVERS = ["cg-jacobi", "cg-single-reduction", "bcgs", "chebyshev", "cg-mg"]


@GN
@pytest.mark.parametrize("solver", SOLVERS)
def test_poisson_solve(ctx, gname, solver):
    """b is an input, x an output: k_cg_init reads b and k_cg_finish writes x with pairs where nx is even and the base aligned (unpadded_pairs);
    B and D on G1 - G4 take the other branch.  Every placement's answer is held to the oracle as the solver's own test holds it."""
    c = ctx(gname)
    P, g, S, N, ns = c.P, c.g, c.S, c.N, c.nullspace
    b = c.b()
    if solver == "cg-jacobi":
        rtol = 1e-5
        xo, io = S.solve(b, ksp=fo.KSP_CG, pc=fo.PC_JACOBI, norm=fo.NORM_PRECONDITIONED, nullspace=ns, rtol=rtol, maxit=10000)
        kw = dict(type=0, pc=fo.PC_JACOBI, norm_type=fo.NORM_PRECONDITIONED, remove_nullspace=int(ns), rtol=rtol, maxit=10000, check_every=7)
        verify = lambda res, what: check_cg(c, b, xo, io, res, rtol, what)
    elif solver == "cg-single-reduction":
        if not ns:
            b = mean_free_rhs(S, N)[1]                          # the right-hand side of tests/test_gpu_cg_single_reduction.py on every grid
        xo, io = S.solve(b, pc=fo.PC_JACOBI, nullspace=ns, rtol=1e-8, maxit=2000, single_reduction=True)
        kw = dict(pc=fo.PC_JACOBI, remove_nullspace=int(ns), rtol=1e-8, maxit=2000, cg_single_reduction=1, check_every=7)

        def verify(res, what):                                  # tests/test_gpu_cg_single_reduction.py:30-34
            assert res["reason"] == io["reason"] and abs(res["iters"] - io["iters"]) <= 2, (what, res["iters"], io["iters"])
            m = min(len(res["history"]), len(io["history"]), 12)
            assert np.allclose(res["history"][:m], io["history"][:m], rtol=1e-6), what
            xg, xr = res["x"], xo
            if ns:
                xg, xr = xg - xg.mean(), xr - xr.mean()
            assert np.linalg.norm(xg - xr) <= 1e-6 * max(np.linalg.norm(xo), 1e-300), what
    elif solver == "bcgs":
        rtol = 1e-6
        xo, io = S.solve(b, ksp=fo.KSP_BCGS, pc=fo.PC_JACOBI, nullspace=ns, rtol=rtol, maxit=2000)
        xr, _ = S.solve(b, ksp=fo.KSP_BCGS, pc=fo.PC_JACOBI, nullspace=ns, rtol=1e-11, maxit=4000)
        kw = dict(type=1, pc=fo.PC_JACOBI, remove_nullspace=int(ns), rtol=rtol, maxit=2000, check_every=5)

        def verify(res, what):                                  # tests/test_gpu_ksp.py:47-71
            assert res["reason"] == io["reason"], what
            m = min(len(res["history"]), len(io["history"]))
            assert np.allclose(res["history"][:3], io["history"][:3], rtol=1e-9), what
            k = min(m, 10)
            assert np.allclose(res["history"][:k], io["history"][:k], rtol=1e-5), what
            drift = max(4, io["iters"] // 6)
            assert abs(res["iters"] - io["iters"]) <= drift, (what, res["iters"], io["iters"])
            eg_, eo_ = np.minimum.accumulate(res["history"]), np.minimum.accumulate(io["history"])
            for a_, b_ in ((eg_, eo_), (eo_, eg_)):
                for k_ in range(len(b_)):
                    assert a_[min(k_ + drift, len(a_) - 1)] <= 10.0 * b_[k_], (what, k_)
            xg = res["x"]
            bn = np.linalg.norm(b)
            assert np.linalg.norm(b - S.mult(xg)) / bn <= 20 * max(np.linalg.norm(b - S.mult(xo)) / bn, rtol), what
            a3 = [xg, xo, xr]
            if ns:
                a3 = [a - a.mean() for a in a3]
            eg, eo = np.linalg.norm(a3[0] - a3[2]), np.linalg.norm(a3[1] - a3[2])
            assert eg <= 5 * max(eo, 1e-5 * np.linalg.norm(a3[2])), (what, eg, eo)
    elif solver == "chebyshev":
        lam = S.gershgorin(fo.PC_JACOBI)
        emin, emax = 0.1 * lam, 1.1 * lam
        xo, io = S.solve(b, ksp=fo.KSP_CHEBYSHEV, pc=fo.PC_JACOBI, norm=fo.NORM_PRECONDITIONED, nullspace=ns, rtol=1e-3, maxit=60, emin=emin, emax=emax)
        kw = dict(type=2, pc=fo.PC_JACOBI, norm_type=fo.NORM_PRECONDITIONED, remove_nullspace=int(ns), rtol=1e-3, maxit=60, emin=emin, emax=emax, check_every=7)

        def verify(res, what):                                  # tests/test_gpu_ksp.py:96-102
            assert res["reason"] == io["reason"] and res["iters"] == io["iters"], (what, res["reason"], io["reason"], res["iters"], io["iters"])
            m = min(len(res["history"]), len(io["history"]))
            assert np.allclose(res["history"][:m], io["history"][:m], rtol=1e-8, atol=1e-300), what
            assert np.linalg.norm(res["x"] - xo) <= 1e-9 * max(np.linalg.norm(xo), 1e-300), what
    else:
        from tests.test_gpu_mg import _bounds
        mg = fo.MgOracle(g, nullspace=ns)
        one_level = mg.nlevels == 1       # G1 and G5: no axis is halved, the "cycle" is the coarse solve on the fine handle itself
        assert one_level == (gname in ("G1", "G5"))
        p = np.random.default_rng(3).standard_normal(N)
        if ns:
            p -= p.mean()
        b = S.mult(p)
        maxit = 100 if one_level else 50
        if not one_level:
            mg = fo.MgOracle(g, nullspace=ns, bounds=_bounds(mg), prolong="linear")
        xo, io = mg.pcg(b, rtol=1e-8, maxit=maxit)
        kw = dict(type=0, pc=2, remove_nullspace=int(ns), rtol=1e-8, maxit=maxit)

        def verify(res, what):                                  # tests/test_gpu_mg.py:56-67; one level: tests/test_gpu_mg.py:114-118
            assert res["reason"] == io["reason"] == 2, (what, res["reason"], io["reason"])
            assert abs(res["iters"] - io["iters"]) <= 1, (what, res["iters"], io["iters"])
            if one_level:
                xg = res["x"]
                assert np.linalg.norm(b - S.mult(xg)) / np.linalg.norm(b) < 1e-6, what
                assert np.linalg.norm((xg - xg.mean()) - xo) <= 1e-5 * np.linalg.norm(xo), what
                return
            m = min(len(res["history"]), len(io["history"]))
            assert np.allclose(res["history"][:3], io["history"][:3], rtol=1e-6), what
            assert np.allclose(res["history"][:m], io["history"][:m], rtol=5e-2), what
            xg = res["x"]
            assert np.linalg.norm(b - S.mult(xg)) / np.linalg.norm(b) < 1e-6, what
            if ns:
                xg = xg - xg.mean()
            assert np.linalg.norm(xg - xo) <= 1e-6 * np.linalg.norm(xo), what

    def call(T):
        _, info = P.solve(T["b"], x=T["x"], history=True, **kw)
        return solve_extras(info)
    drive(f"{gname} fl_poisson_solve {solver}", [("b", N, "in"), ("x", N, "out")], {"b": b}, call, ["x"], verify=verify, nx=c.n[0], P=P, fns=["fl_poisson_solve"])


# ------------------------------------------------------------------------------------------------------------------ the momentum block

@GN
def test_momentum_apply_diagonal_rowsum(ctx, gname):
    """y = A v stored by k_mom2 (ny <= 8) or k_mom3 (ny > 8, the state handed over with v0) with pairs where nx is even and y's base aligned
    (mom_apply_t); B, C and D take the other branch.  Tolerance: _close of tests/test_gpu_momentum.py (2e-13 of the largest entry)."""
    c = ctx(gname)
    M, N = c.M, c.N
    A = c.cheb_state()
    v = np.random.default_rng(11).standard_normal(3 * N)
    want = A.mult(v)
    drive(f"{gname} fl_momentum_apply", [("v", 3 * N, "in"), ("y", 3 * N, "out")], {"v": v}, quiet(lambda T: M.apply(T["v"], T["y"])), ["y"],
          placements=ABCD, verify=lambda res, what: close(res["y"], want), nx=c.n[0], P=c.P, fns=["fl_momentum_apply"])
    # the state itself on caller arrays: fl_momentum_set_state_v0 reads the three V0, the nine v0interp and v0
    V0, v0 = c._state[0], c._state[1]
    dt, rho, mu = c._state[2:5]
    W = c.g.apply_B(v0)
    nf = c.nface
    spec = ([(f"V0{d}", nf[d], "in") for d in range(3)] + [(f"W{q}", nf[q % 3], "in") for q in range(9)] + [("v0", 3 * N, "in"), ("v", 3 * N, "in"), ("y", 3 * N, "out")])
    inputs = {**{f"V0{d}": V0[d] for d in range(3)}, **{f"W{q}": W[q] for q in range(9)}, "v0": v0, "v": v}

    def with_state(T):
        M.set_state(dt, rho, mu, [T[f"V0{d}"] for d in range(3)], [T[f"W{q}"] for q in range(9)], v0=T["v0"])
        T.release(*[f"V0{d}" for d in range(3)], *[f"W{q}" for q in range(9)], "v0")         # copied: the caller reuses its buffers
        M.apply(T["v"], T["y"])
    try:
        drive(f"{gname} fl_momentum_set_state_v0 + apply", spec, inputs, with_state, ["y"], verify=lambda res, what: close(res["y"], want), nx=c.n[0],
              P=c.P, fns=["fl_momentum_set_state_v0", "fl_momentum_apply"])
    finally:
        c.cheb_state()                                          # the handle keeps no pointer into an arena that is gone
    A2, dt2, rho2, mu2 = c.abf_state()                          # the stored state: k_mom2 on every grid
    want2 = A2.mult(v)
    V02, W2 = c._abf[0], c._abf[1]                              # ... and fl_momentum_set_state itself on caller arrays
    spec = [(f"V0{d}", nf[d], "in") for d in range(3)] + [(f"W{q}", nf[q % 3], "in") for q in range(9)] + [("v", 3 * N, "in"), ("y", 3 * N, "out")]
    inputs = {**{f"V0{d}": V02[d] for d in range(3)}, **{f"W{q}": W2[q] for q in range(9)}, "v": v}

    def with_stored_state(T):
        M.set_state(dt2, rho2, mu2, [T[f"V0{d}"] for d in range(3)], [T[f"W{q}"] for q in range(9)])
        T.release(*[f"V0{d}" for d in range(3)], *[f"W{q}" for q in range(9)])
        M.apply(T["v"], T["y"])
    try:
        drive(f"{gname} fl_momentum_set_state + apply", spec, inputs, with_stored_state, ["y"], verify=lambda res, what: close(res["y"], want2), nx=c.n[0],
              P=c.P, fns=["fl_momentum_set_state", "fl_momentum_apply"])
    finally:
        c.abf_state()
    drive(f"{gname} fl_momentum_apply stored", [("v", 3 * N, "in"), ("y", 3 * N, "out")], {"v": v}, quiet(lambda T: M.apply(T["v"], T["y"])), ["y"],
          placements=ABCD, verify=lambda res, what: close(res["y"], want2), nx=c.n[0], P=c.P, fns=["fl_momentum_apply"])
    drive(f"{gname} fl_momentum_diagonal", [("d", 3 * N, "out")], {}, lambda T: raw(c.P, "fl_momentum_diagonal", M.h, ptr(T["d"])), ["d"],
          verify=lambda res, what: close(res["d"], A2.diag()), nx=c.n[0], P=c.P, fns=["fl_momentum_diagonal"])
    ones = A2.mult(np.ones(3 * N))
    drive(f"{gname} fl_momentum_rowsum", [("d", 3 * N, "out")], {}, lambda T: raw(c.P, "fl_momentum_rowsum", M.h, ptr(T["d"])), ["d"],
          verify=lambda res, what: close(res["d"], ones), nx=c.n[0], P=c.P, fns=["fl_momentum_rowsum"])


MOM_SOLVERS = ["bcgs", "gmres", "chebyshev", "chebyshev-guess"]


@GN
@pytest.mark.parametrize("solver", MOM_SOLVERS)
def test_momentum_solve(ctx, gname, solver):
    """b is read by k_mom_pw3 with pairs where nx is even and b's base aligned (mom_pw); x is written by the update kernels.  Chebyshev from a
    non-zero guess: x is inout."""
    c = ctx(gname)
    M, N = c.M, c.N
    A = c.cheb_state()
    b = np.random.default_rng(7).standard_normal(3 * N)
    spec, inputs, x_role = [("b", 3 * N, "in"), ("x", 3 * N, "out")], {"b": b}, "out"
    if solver == "bcgs":
        rtol = 1e-8
        xo, io = A.solve(b, ksp=fo.KSP_BCGS, pc=fo.PC_JACOBI, nullspace=False, rtol=rtol, maxit=500)
        kw = dict(pc=fo.PC_JACOBI, rtol=rtol, maxit=500)

        def verify(res, what):                                  # tests/test_gpu_momentum.py:94-102
            assert io["reason"] > 0 and res["reason"] == io["reason"], what
            m = min(len(res["history"]), len(io["history"]))
            assert np.allclose(res["history"][:3], io["history"][:3], rtol=1e-9), what
            assert np.allclose(res["history"][:min(m, 8)], io["history"][:min(m, 8)], rtol=1e-5), what
            assert abs(res["iters"] - io["iters"]) <= max(2, io["iters"] // 6), what
            assert np.linalg.norm(b - A.mult(res["x"])) <= 50 * rtol * np.linalg.norm(b), what
            assert np.linalg.norm(res["x"] - xo) <= 1e-5 * np.linalg.norm(xo), what
    elif solver == "gmres":
        from fluca_amd import capi
        rtol, restart = 1e-8, 5
        xo, io = fo.gmres(A, b, pc=fo.PC_JACOBI, rtol=rtol, restart=restart, maxit=300)
        kw = dict(type=capi.KSP_GMRES, pc=fo.PC_JACOBI, rtol=rtol, maxit=300, gmres_restart=restart)

        def verify(res, what):                                  # tests/test_gpu_momentum.py:525-529
            assert res["reason"] == io["reason"] == 2, what
            assert abs(res["iters"] - io["iters"]) <= 1, (what, res["iters"], io["iters"])
            m = min(len(res["history"]), len(io["history"]))
            assert np.allclose(res["history"][:m], io["history"][:m], rtol=1e-6, atol=1e-12 * io["history"][0]), what
            assert np.linalg.norm(res["x"] - xo) <= 1e-6 * np.linalg.norm(xo), what
    elif solver == "chebyshev":
        emin, emax = M.chebyshev_interval()
        rtol = 1e-8
        xo, io = A.solve(b, ksp=fo.KSP_CHEBYSHEV, pc=fo.PC_JACOBI, norm=fo.NORM_PRECONDITIONED, nullspace=False, rtol=rtol, maxit=400, emin=emin, emax=emax)
        kw = dict(type=fo.KSP_CHEBYSHEV, pc=fo.PC_JACOBI, norm_type=fo.NORM_PRECONDITIONED, rtol=rtol, maxit=400, check_every=5)

        def verify(res, what):                                  # tests/test_gpu_momentum_cheb.py:56-59
            assert io["reason"] > 0 and res["reason"] == io["reason"], what
            assert res["iters"] == io["iters"], (what, res["iters"], io["iters"])
            k = io["iters"] + 1
            assert np.allclose(res["history"][:k], io["history"][:k], rtol=1e-8, atol=1e-13 * io["history"][0]), what
            assert np.linalg.norm(res["x"] - xo) <= 1e-9 * np.linalg.norm(xo), what
    else:
        rtol = 1e-7
        kw = dict(type=fo.KSP_CHEBYSHEV, pc=fo.PC_JACOBI, rtol=rtol, maxit=400, check_every=3, initial_guess_nonzero=1)
        xo, _ = A.solve(b, ksp=fo.KSP_BCGS, pc=fo.PC_JACOBI, nullspace=False, rtol=1e-13, maxit=1000)
        dinv = 1.0 / A.diag()
        bnorm = np.linalg.norm(dinv * b)
        rng = np.random.default_rng(9)
        guess = xo + 1e-3 * np.linalg.norm(xo) / np.sqrt(xo.size) * rng.standard_normal(xo.size)
        _, plain = M.solve(dev(b), type=fo.KSP_CHEBYSHEV, pc=fo.PC_JACOBI, rtol=rtol, maxit=400, check_every=3)
        spec, inputs = [("b", 3 * N, "in"), ("x", 3 * N, "inout")], {"b": b, "x": guess}

        def verify(res, what):                                  # tests/test_gpu_momentum_cheb.py:157-161, case (b)
            assert res["reason"] == 2 and 0 < res["iters"] < plain["iters"], (what, res["iters"], plain["iters"])
            assert np.linalg.norm(dinv * (b - A.mult(res["x"]))) / bnorm <= 1.01 * rtol, what
            assert np.linalg.norm(res["x"] - xo) <= 50 * rtol * np.linalg.norm(xo), what
            assert abs(res["rnorm0"] - bnorm) <= 1e-10 * bnorm, what

    def call(T):
        _, info = M.solve(T["b"], x=T["x"], history=True, **kw)
        return solve_extras(info)
    drive(f"{gname} fl_momentum_solve {solver}", spec, inputs, call, ["x"], verify=verify, nx=c.n[0], P=c.P, fns=["fl_momentum_solve"])


@GN
def test_face_interp_and_interp_faces(ctx, gname):
    c = ctx(gname)
    P, M, g, N, n = c.P, c.M, c.g, c.N, c.n
    c.cheb_state()
    rng = np.random.default_rng(21)
    v = rng.standard_normal(3 * N)
    rhs = [rng.standard_normal(g.nface[d]) for d in range(3)]
    want = g.apply_T(v, rhs)
    spec = [("v", 3 * N, "in")] + [(f"rhs{d}", g.nface[d], "in") for d in range(3)] + [(f"V{d}", g.nface[d], "out") for d in range(3)]

    def verify(res, what):                                      # tests/test_gpu_momentum.py:144-145
        for d in range(3):
            close(res[f"V{d}"], want[d])
    drive(f"{gname} fl_momentum_face_interp", spec, {"v": v, **{f"rhs{d}": rhs[d] for d in range(3)}},
          lambda T: raw(P, "fl_momentum_face_interp", M.h, ptr(T["v"]), ptrs([T[f"rhs{d}"] for d in range(3)]), ptrs([T[f"V{d}"] for d in range(3)])),
          [f"V{d}" for d in range(3)], verify=verify, nx=n[0], P=P, fns=["fl_momentum_face_interp"])
    # V_d = rhs_d + alpha (T v)_d with rhs aliasing V, as NSFormFunction calls it (tests/test_gpu_step_rhs.py:383-385)
    alpha, Tv = -1.0, g.apply_T(v)
    spec = [("v", 3 * N, "in")] + [(f"V{d}", g.nface[d], "inout") for d in range(3)]

    def scaled(T):
        three = ptrs([T[f"V{d}"] for d in range(3)])
        raw(P, "fl_momentum_face_interp_scaled", M.h, alpha, ptr(T["v"]), three, three)

    def verify_scaled(res, what):
        for d in range(3):
            close(res[f"V{d}"], rhs[d] + alpha * Tv[d])
    drive(f"{gname} fl_momentum_face_interp_scaled", spec, {"v": v, **{f"V{d}": rhs[d] for d in range(3)}}, scaled, [f"V{d}" for d in range(3)],
          verify=verify_scaled, nx=n[0], P=P, fns=["fl_momentum_face_interp_scaled"])
    # cnl->v0interp = B v + vbc: nine face arrays, [c * 3 + d] = component c on the d-faces
    wantB = g.apply_B(v)
    vbc = [rng.standard_normal(g.nface[q % 3]) for q in range(9)]
    spec = [("v", 3 * N, "in")] + [(f"vbc{q}", g.nface[q % 3], "in") for q in range(9)] + [(f"W{q}", g.nface[q % 3], "out") for q in range(9)]

    def verify_B(res, what):                                    # tests/test_gpu_momentum.py:370-372
        for q in range(9):
            assert np.abs(res[f"W{q}"] - (wantB[q] + vbc[q])).max() <= 2e-13 * max(np.abs(v).max(), np.abs(vbc[q]).max()), (what, q)
    drive(f"{gname} fl_momentum_interp_faces", spec, {"v": v, **{f"vbc{q}": vbc[q] for q in range(9)}},
          quiet(lambda T: M.interp_faces(T["v"], [T[f"vbc{q}"] for q in range(9)], out=[T[f"W{q}"] for q in range(9)])),
          [f"W{q}" for q in range(9)], verify=verify_B, nx=n[0], P=P, fns=["fl_momentum_interp_faces"])
    # ends only: the faces at the two ends of each axis are written; an inner entry keeps what it held or takes the value of the whole field
    junk = [rng.standard_normal(g.nface[q % 3]) for q in range(9)]
    spec = [("v", 3 * N, "in")] + [(f"vbc{q}", g.nface[q % 3], "in") for q in range(9)] + [(f"W{q}", g.nface[q % 3], "inout") for q in range(9)]
    nf = [int(g.nface[d]) // (N // n[d]) for d in range(3)]

    def verify_ends(res, what):
        for q in range(9):
            d = q % 3
            shp = [n[2], n[1], n[0]]
            shp[2 - d] = nf[d]
            got, full, old = res[f"W{q}"].reshape(shp), (wantB[q] + vbc[q]).reshape(shp), junk[q].reshape(shp)
            tol = 2e-13 * max(np.abs(v).max(), np.abs(vbc[q]).max())
            written = np.abs(got - full) <= tol
            assert (written | (bits(got) == bits(old))).all(), (what, q)
            if c.bc[2 * d] != PER:
                for side in (0, 1):
                    assert written[layer(shp, d, side)].all(), (what, q, side)
    drive(f"{gname} fl_momentum_interp_faces_ends", spec, {"v": v, **{f"vbc{q}": vbc[q] for q in range(9)}, **{f"W{q}": junk[q] for q in range(9)}},
          quiet(lambda T: M.interp_faces(T["v"], [T[f"vbc{q}"] for q in range(9)], ends_only=True, out=[T[f"W{q}"] for q in range(9)])),
          [f"W{q}" for q in range(9)], verify=verify_ends, nx=n[0], P=P, fns=["fl_momentum_interp_faces_ends"])


@GN
def test_momentum_rhs_and_jacobian_mult(ctx, gname):
    c = ctx(gname)
    P, M, g, N = c.P, c.M, c.g, c.N
    A, _, _, _ = c.abf_state()
    # fl_momentum_rhs = v0 + cv L v0 - kappa G p + vbc, per entry to 2e-13 x the sum of the terms' magnitudes (tests/test_gpu_step_rhs.py:401-413)
    dt_r, rho_r, mu_r = 0.013, 13.0, 0.4                        # dt / rho = the handle's kappa
    so = fo.StepOracle(g, dt_r, rho_r, mu_r)
    cv = 0.5 * mu_r * dt_r / rho_r
    rng = np.random.default_rng(29)
    v0, p, vbc = rng.standard_normal(3 * N), rng.standard_normal(N), rng.standard_normal(3 * N)
    want = v0 + cv * so.L.mult(v0) - np.concatenate(g.apply_G(p)) + vbc
    scale = sr.momrhs_scale(so, v0, p, vbc)
    drive(f"{gname} fl_momentum_rhs", [("v0", 3 * N, "in"), ("p", N, "in"), ("vbc", 3 * N, "in"), ("out", 3 * N, "out")], dict(v0=v0, p=p, vbc=vbc),
          quiet(lambda T: M.rhs(dt_r, rho_r, mu_r, T["v0"], T["p"], T["vbc"], out=T["out"])), ["out"],
          verify=lambda res, what: sr.within(res["out"], want, scale, 2e-13, what), nx=c.n[0], P=P, fns=["fl_momentum_rhs"])
    # the block Jacobian (tests/test_gpu_momentum.py:319-330)
    rng = np.random.default_rng(41)
    v = rng.standard_normal(3 * N)
    Vf = [rng.standard_normal(g.nface[d]) for d in range(3)]
    p = rng.standard_normal(N)
    kGp = np.concatenate(g.apply_G(p))
    Tw, kGst = g.apply_T(v + kGp), g.apply_gst(p)
    fv_ref, fV_ref, fp_ref = A.mult(v) + kGp, [Vf[d] - Tw[d] + kGst[d] for d in range(3)], -g.rhs(*Vf)
    spec = ([("v", 3 * N, "in")] + [(f"V{d}", g.nface[d], "in") for d in range(3)] + [("p", N, "in"), ("fv", 3 * N, "out")] +
            [(f"fV{d}", g.nface[d], "out") for d in range(3)] + [("fp", N, "out")])

    def verify(res, what):
        close(res["fv"], fv_ref)
        close(res["fp"], fp_ref, 1e-12)
        for d in range(3):
            close(res[f"fV{d}"], fV_ref[d], 1e-12)
    drive(f"{gname} fl_abf_jacobian_mult", spec, {"v": v, "p": p, **{f"V{d}": Vf[d] for d in range(3)}},
          lambda T: raw(P, "fl_abf_jacobian_mult", M.h, ptr(T["v"]), ptrs([T[f"V{d}"] for d in range(3)]), ptr(T["p"]), ptr(T["fv"]),
                        ptrs([T[f"fV{d}"] for d in range(3)]), ptr(T["fp"])),
          ["fv", "fp"] + [f"fV{d}" for d in range(3)], verify=verify, nx=c.n[0], P=P, fns=["fl_abf_jacobian_mult"])


@GN
@pytest.mark.parametrize("kind", ["ID", "DIAG"])
def test_schur_apply(ctx, gname, kind):
    """fl_abf_schur_apply: ID is the 7-point operator of the hot path (2e-13), DIAG the one-pass variable-coefficient product (2e-10: the oracle's
    composition cancels, tests/test_gpu_momentum.py:234-247)"""
    c = ctx(gname)
    P, M, g, N = c.P, c.M, c.g, c.N
    A, _, _, _ = c.abf_state()
    p = np.random.default_rng(17).standard_normal(N)
    if kind == "ID":
        want, tol = c.S.mult(p), 2e-13
        M.set_ainv_types(schur=fo.AINV_ID)
    else:
        want, tol = fo.abf_schur_apply(g, fo.abf_ainv(A, fo.AINV_DIAG), p), 2e-10
        M.set_ainv_types(schur=fo.AINV_DIAG)
    try:
        drive(f"{gname} fl_abf_schur_apply {kind}", [("p", N, "in"), ("y", N, "out")], {"p": p},
              lambda T: raw(P, "fl_abf_schur_apply", M.h, ptr(T["p"]), ptr(T["y"])), ["y"], verify=lambda res, what: close(res["y"], want, tol), nx=c.n[0],
              P=P, fns=["fl_abf_schur_apply"])
    finally:
        M.set_ainv_types(schur=fo.AINV_ID)


@GN
def test_abf_apply(ctx, gname):
    """PCApply_ABF: two solves, the face interpolation, the Schur right-hand side and the projection of all six arrays on the caller's v, V and p
    (tests/test_gpu_momentum.py:182-204)"""
    from fluca_amd import capi
    from fluca_amd.poisson import KspOptions
    c = ctx(gname)
    P, M, g, N, n, ns = c.P, c.M, c.g, c.N, c.n, c.nullspace
    rng = np.random.default_rng(31)
    V0 = [rng.standard_normal(g.nface[d]) for d in range(3)]
    W = [rng.standard_normal(g.nface[d]) for q in range(9) for d in [q % 3]]
    rho, mu = 1.0, 0.5 * min(np.diff(g.xf[d]).min() for d in range(3))
    dt = g.kappa * rho
    c.keep = [[dev(a) for a in V0], [dev(a) for a in W]]
    M.set_state(dt, rho, mu, c.keep[0], c.keep[1])
    M.set_ainv_types(schur=fo.AINV_ID, upper=fo.AINV_ID)
    A = g.assemble_momentum(1.0, dt, -0.5 * mu * dt / rho, V0, W)
    S = c.S
    momrhs = rng.standard_normal(3 * N)
    interprhs = [1e-2 * rng.standard_normal(g.nface[d]) for d in range(3)]
    nf = [int(g.nface[d]) // (N // n[d]) for d in range(3)]
    if ns:          # no flux through the walls: a singular S needs a right-hand side without a constant component
        for d in range(3):
            if c.bc[2 * d] != PER:
                shp = [n[2], n[1], n[0]]
                shp[2 - d] = nf[d]
                a = interprhs[d].reshape(shp)
                a[layer(shp, d, 0)] = 0.0
                a[layer(shp, d, 1)] = 0.0
    vs, i0 = A.solve(momrhs, ksp=fo.KSP_BCGS, pc=fo.PC_JACOBI, nullspace=False, rtol=1e-10, maxit=500)
    Vs = g.apply_T(vs, interprhs)
    srhs = g.rhs(*Vs)
    po, i1 = S.solve(srhs, ksp=fo.KSP_CG, pc=fo.PC_JACOBI, nullspace=ns, rtol=1e-10, maxit=5000)
    Gp, Gst = g.apply_G(po), g.apply_gst(po)
    v_ref, V_ref = vs - np.concatenate(Gp), [Vs[d] - Gst[d] for d in range(3)]
    mo = KspOptions(type=capi.KSP_BCGS, rtol=1e-10, maxit=500)
    so = KspOptions(rtol=1e-10, maxit=5000, remove_nullspace=int(ns))
    spec = ([("momrhs", 3 * N, "in")] + [(f"ir{d}", g.nface[d], "in") for d in range(3)] + [("v", 3 * N, "out")] +
            [(f"V{d}", g.nface[d], "out") for d in range(3)] + [("p", N, "out")])

    def call(T):
        st = (capi.fl_ksp_stats * 2)()
        raw(P, "fl_abf_apply", M.h, C.byref(mo.o), C.byref(so.o), ptr(T["momrhs"]), ptrs([T[f"ir{d}"] for d in range(3)]), None, ptr(T["v"]),
            ptrs([T[f"V{d}"] for d in range(3)]), ptr(T["p"]), st)
        return dict(iters=[st[0].iters, st[1].iters], reason=[st[0].reason, st[1].reason])

    def verify(res, what):
        assert list(res["reason"]) == [i0["reason"], i1["reason"]], what
        assert abs(res["iters"][0] - i0["iters"]) <= 2 and abs(res["iters"][1] - i1["iters"]) <= max(3, i1["iters"] // 20), (what, res["iters"], i0["iters"], i1["iters"])
        pg, pr = res["p"], po
        if ns:
            pg, pr = pg - pg.mean(), pr - pr.mean()
        assert np.linalg.norm(pg - pr) <= 1e-6 * np.linalg.norm(pr), what
        assert np.linalg.norm(res["v"] - v_ref) <= 1e-7 * np.linalg.norm(v_ref), what
        for d in range(3):
            assert np.linalg.norm(res[f"V{d}"] - V_ref[d]) <= 1e-7 * max(np.linalg.norm(V_ref[d]), 1e-30), (what, d)
    drive(f"{gname} fl_abf_apply", spec, {"momrhs": momrhs, **{f"ir{d}": interprhs[d] for d in range(3)}}, call,
          ["v", "p"] + [f"V{d}" for d in range(3)], verify=verify, nx=n[0], P=P, fns=["fl_abf_apply"])


@GN
def test_add_buoyancy(ctx, gname):
    """fl_momentum_add_buoyancy: the sixth dispatch (the kernel's `vec` mask takes 16-byte accesses per component and scalar where its base is
    aligned).  Three scalars, gravity on two axes; the cell-by-cell bound and bit checks of tests/test_gpu_buoyancy.py::check."""
    from tests.test_gpu_buoyancy import DT, check, coefficients, fields
    c = ctx(gname)
    M, N = c.M, c.N
    accel, refs = coefficients("three-scalars-two-axes", np.random.default_rng(11))
    phis, m = fields(c.n, 3, 3)
    spec = [("momrhs", 3 * N, "inout")] + [(f"phi{s}", N, "in") for s in range(3)]
    drive(f"{gname} fl_momentum_add_buoyancy", spec, {"momrhs": m, **{f"phi{s}": phis[s] for s in range(3)}},
          quiet(lambda T: M.add_buoyancy(T["momrhs"], [T[f"phi{s}"] for s in range(3)], accel, refs, DT)), ["momrhs"], placements=ABCD,
          verify=lambda res, what: check(res["momrhs"], m, phis, accel, refs, DT, what), nx=c.n[0], P=c.P, fns=["fl_momentum_add_buoyancy"])


# ------------------------------------------------------------------------------------------------------------------ BLAS-1

@GN
def test_vec_lincomb(ctx, gname):
    """y = a x + b z on momentum-sized vectors; y aliasing x and y aliasing z, which the header allows (tests/test_gpu_step_rhs.py:314-326)"""
    c = ctx(gname)
    P, m = c.P, 3 * c.N
    rng = np.random.default_rng(m)
    x, z = rng.uniform(0.5, 1.5, m), rng.uniform(0.5, 1.5, m)
    lin = lambda a, xx, b, zz, yy: raw(P, "fl_vec_lincomb", P.h, m, a, ptr(xx), b, ptr(zz), ptr(yy))
    LC = dict(P=P, fns=["fl_vec_lincomb"])
    for a, b in ((-1.0, 1.0), (2.0, -1.0)):     # exact products: one rounding, fused or not
        drive(f"{gname} fl_vec_lincomb {a} {b}", [("x", m, "in"), ("z", m, "in"), ("y", m, "out")], dict(x=x, z=z), lambda T: lin(a, T["x"], b, T["z"], T["y"]),
              ["y"], placements=ABCD, verify=lambda res, what: same_bits(res["y"], a * x + b * z) or pytest.fail(what), nx=c.n[0], **LC)
    a, b = 1.7, 0.6
    cands = [a * x + b * z, sr.fused(a, x, b * z), sr.fused(b, z, a * x)]
    drive(f"{gname} fl_vec_lincomb general", [("x", m, "in"), ("z", m, "in"), ("y", m, "out")], dict(x=x, z=z), lambda T: lin(a, T["x"], b, T["z"], T["y"]),
          ["y"], placements=ABCD, verify=lambda res, what: sr.one_ulp_of_any(res["y"], cands, what), nx=c.n[0], **LC)
    drive(f"{gname} fl_vec_lincomb y = x", [("x", m, "inout"), ("z", m, "in")], dict(x=x, z=z), lambda T: lin(a, T["x"], b, T["z"], T["x"]),
          ["x"], placements=ABCD, verify=lambda res, what: sr.one_ulp_of_any(res["x"], cands, what), nx=c.n[0], **LC)
    drive(f"{gname} fl_vec_lincomb y = z", [("x", m, "in"), ("z", m, "inout")], dict(x=x, z=z), lambda T: lin(a, T["x"], b, T["z"], T["z"]),
          ["z"], placements=ABCD, verify=lambda res, what: sr.one_ulp_of_any(res["z"], cands, what), nx=c.n[0], **LC)


@GN
def test_vec_dot_mdot_maxpy(ctx, gname):
    c = ctx(gname)
    P, m, k = c.P, 3 * c.N, 11                   # more vectors than one launch takes (8)
    rng = np.random.default_rng(m + 1)
    x, y = rng.standard_normal(m), rng.standard_normal(m)
    pr, e = sr.two_prod(x, y)
    exact = math.fsum(np.concatenate([pr, e]))
    bound = m * 2.0 ** -53 * float(np.abs(pr).sum())            # tests/test_gpu_step_rhs.py:352-359

    def dot(T):
        out = C.c_double(np.nan)
        raw(P, "fl_vec_dot", P.h, m, ptr(T["x"]), ptr(T["y"]), C.byref(out))
        return {"dot": out.value}
    drive(f"{gname} fl_vec_dot", [("x", m, "in"), ("y", m, "in")], dict(x=x, y=y), dot, [],
          verify=lambda res, what: abs(res["dot"] - exact) <= bound or pytest.fail(f"{what}: {res['dot']!r} {exact!r}"), nx=c.n[0], P=P, fns=["fl_vec_dot"])
    Y = rng.standard_normal((k, m))
    spec = [("x", m, "inout")] + [(f"Y{j}", m, "in") for j in range(k)]
    inputs = {"x": x, **{f"Y{j}": Y[j] for j in range(k)}}

    def mdot(T):
        out = (C.c_double * k)()
        raw(P, "fl_vec_mdot", P.h, m, ptr(T["x"]), ptrs([T[f"Y{j}"] for j in range(k)]), k, out)
        return {"mdot": np.array(out[:])}
    drive(f"{gname} fl_vec_mdot", spec, inputs, mdot, [],       # tests/test_gpu_momentum.py:498
          verify=lambda res, what: np.allclose(res["mdot"], Y @ x, rtol=1e-12, atol=1e-12) or pytest.fail(what), nx=c.n[0], P=P, fns=["fl_vec_mdot"])
    a = rng.standard_normal(k)
    drive(f"{gname} fl_vec_maxpy", spec, inputs,
          lambda T: raw(P, "fl_vec_maxpy", P.h, m, ptr(T["x"]), (C.c_double * k)(*a), ptrs([T[f"Y{j}"] for j in range(k)]), k), ["x"],
          verify=lambda res, what: np.allclose(res["x"], x + a @ Y, rtol=1e-13, atol=1e-13) or pytest.fail(what), nx=c.n[0],
          P=P, fns=["fl_vec_maxpy"])     # :502


# ------------------------------------------------------------------------------------------------------------------ layout conversions

@GN
def test_layout_conversions(ctx, gname):
    """fl_layout_{from,to}_dmstag_{global,local} on one rank, against the enumeration of tests/test_gpu_layout.py (exact copies)"""
    from fluca_amd import capi
    from tests.test_gpu_layout import BACK, DOWN, ELEM, LEFT, enumerate_global
    c = ctx(gname)
    P, n, N = c.P, c.n, c.N
    nel = list(n)
    extra = [c.bc[2 * d] != PER for d in range(3)]
    ext = {ELEM: nel, LEFT: [nel[0] + extra[0], nel[1], nel[2]], DOWN: [nel[0], nel[1] + extra[1], nel[2]], BACK: [nel[0], nel[1], nel[2] + extra[2]]}
    dof = (0, 0, 2, 1)
    dofc = (C.c_int * 4)(*dof)
    order = enumerate_global(nel, extra, dof)
    ent = C.c_int64()
    capi.check(capi.lib.fl_dmstag_global_entries(P.h, dofc, C.byref(ent)))
    assert ent.value == len(order)
    rng = np.random.default_rng(1)
    glob = rng.standard_normal(len(order))
    for what, comp in ((ELEM, 0), (LEFT, 1), (DOWN, 0), (BACK, 1)):
        e = ext[what]
        m = e[0] * e[1] * e[2]
        where = np.array([pos for pos, (w, cc, i, j, k) in enumerate(order) if w == what and cc == comp])
        index = np.array([(k * e[1] + j) * e[0] + i for (w, cc, i, j, k) in order if w == what and cc == comp])
        want = np.empty(m)
        want[index] = glob[where]
        drive(f"{gname} fl_layout_from_dmstag_global {what} {comp}", [("glob", glob.size, "in"), ("out", m, "out")], {"glob": glob},
              lambda T: raw(P, "fl_layout_from_dmstag_global", P.h, dofc, what, comp, ptr(T["glob"]), ptr(T["out"])), ["out"],
              verify=lambda res, tag: same_bits(res["out"], want) or pytest.fail(tag), nx=n[0], P=P, fns=["fl_layout_from_dmstag_global"])
        arr = rng.standard_normal(m)
        back = glob.copy()
        back[where] = arr[index]
        drive(f"{gname} fl_layout_to_dmstag_global {what} {comp}", [("arr", m, "in"), ("glob", glob.size, "inout")], {"arr": arr, "glob": glob},
              lambda T: raw(P, "fl_layout_to_dmstag_global", P.h, dofc, what, comp, ptr(T["arr"]), ptr(T["glob"])), ["glob"],
              verify=lambda res, tag: same_bits(res["glob"], back) or pytest.fail(tag), nx=n[0], P=P, fns=["fl_layout_to_dmstag_global"])
    # DMStagVecGetArray's ghosted box (tests/test_gpu_layout.py:132-163): ten slots per element
    per = [c.bc[2 * d] == PER for d in range(3)]
    gstart = [-1 if per[d] else 0 for d in range(3)]
    gsize = [n[d] + 1 - gstart[d] for d in range(3)]
    D = capi.fl_dmstag_local()
    for d in range(3):
        D.gstart[d], D.gsize[d], D.start[d] = gstart[d], gsize[d], 0
    D.entries = 10
    loc = rng.standard_normal((gsize[2], gsize[1], gsize[0], 10))
    o = [-gstart[d] for d in range(3)]
    for what, slot in ((ELEM, 9), (LEFT, 6), (BACK, 1)):
        e = ext[what]
        m = e[0] * e[1] * e[2]
        box = (slice(o[2], o[2] + e[2]), slice(o[1], o[1] + e[1]), slice(o[0], o[0] + e[0]), slot)
        want = loc[box].ravel()
        drive(f"{gname} fl_layout_from_dmstag_local {what} {slot}", [("loc", loc.size, "in"), ("out", m, "out")], {"loc": loc},
              lambda T: raw(P, "fl_layout_from_dmstag_local", P.h, C.byref(D), what, slot, ptr(T["loc"]), ptr(T["out"])), ["out"],
              verify=lambda res, tag: same_bits(res["out"], want) or pytest.fail(tag), nx=n[0], P=P, fns=["fl_layout_from_dmstag_local"])
        arr = rng.standard_normal(m)
        back = loc.copy()
        back[box] = arr.reshape(back[box].shape)
        drive(f"{gname} fl_layout_to_dmstag_local {what} {slot}", [("arr", m, "in"), ("loc", loc.size, "inout")], {"arr": arr, "loc": loc},
              lambda T: raw(P, "fl_layout_to_dmstag_local", P.h, C.byref(D), what, slot, ptr(T["arr"]), ptr(T["loc"])), ["loc"],
              verify=lambda res, tag: same_bits(res["loc"], back.ravel()) or pytest.fail(tag), nx=n[0], P=P, fns=["fl_layout_to_dmstag_local"])


# ------------------------------------------------------------------------------------------------------------------ immersed boundary

# the grids' own periodic axes where fl_ibm_create takes them -- a periodic axis needs twice the support, 8 cells for Peskin-4 and 6 for Roma-3:
# the 128-cell x of G4; its 4-cell y and the 3-cell z of G3 and G4 are walled -- and walls elsewhere
IBM_BC = {"G1": [V] * 6, "G2": [V] * 6, "G3": [V] * 6, "G4": [PER, PER, V, V, V, V], "G5": [V] * 6}


@GN
@pytest.mark.parametrize("kind", [fo.DELTA_PESKIN4, fo.DELTA_ROMA3], ids=["peskin4", "roma3"])
def test_ibm(gname, kind):
    """fl_ibm_create at one set of positions, fl_ibm_update to another, fl_ibm_interp, fl_ibm_spread and fl_ibm_force (one body) on a replicated set
    of 37 markers, some next to the walls or the periodic seam; all marker arrays stand in the arena.  Interpolation and spreading against the
    oracle at the tolerances of tests/test_gpu_ibm.py:67, 73; force and torque within the bound and with the bits of tests/ibm_force_reference.py
    (tests/test_gpu_ibm_force.py::_check)."""
    from fluca_amd import capi
    from tests import ibm_force_reference as fr
    from tests.test_gpu_ibm import sphere_markers
    n, bc = GRIDS[gname][0], IBM_BC[gname]
    box = [(0.0, 1.0)] * 3
    P, g = make_pair(n, bc, box=box)
    N, L = g.ncell, 37
    X = sphere_markers(L, (0.5, 0.5, 0.5), 0.3)
    X[0][:5] = [0.01, 0.99, 0.5, 0.02, 0.97]
    X[1][:5] = [0.5, 0.5, 0.01, 0.98, 0.03]
    X[2][:5] = [0.03, 0.5, 0.99, 0.5, 0.5]
    rng = np.random.default_rng(4)
    first = [np.clip(a + rng.uniform(-0.05, 0.05, L), 0.005, 0.995) for a in X]       # where the set is created, before fl_ibm_update moves it to X
    u = rng.standard_normal((3, N))
    F = rng.standard_normal((3, L))
    dV = rng.uniform(0.5, 1.5, L) * 1e-3
    f0 = rng.standard_normal((3, N))
    wantU = g.ibm_interp(kind, X, u)
    wantf = g.ibm_spread(kind, X, dV, F, f0.copy())
    about = np.array([0.5, 0.4375, 0.25])
    period = tuple(1.0 if bc[2 * d] == PER else None for d in range(3))
    ref = fr.reference(np.array(X), F, dV, about[None], period)
    spec = ([(f"first{d}", L, "in") for d in range(3)] + [("X0", L, "in"), ("X1", L, "in"), ("X2", L, "in"), ("u", 3 * N, "in"), ("U", 3 * L, "out"),
            ("F", 3 * L, "in"), ("dV", L, "in"), ("f", 3 * N, "inout")])
    inputs = dict(first0=first[0], first1=first[1], first2=first[2], X0=X[0], X1=X[1], X2=X[2], u=u, F=F, dV=dV, f=f0)
    # what a marker position holds while its producer is pending, and again once the set has copied it: OTHER markers inside the box, never a NaN (a
    # position becomes a cell index: misordering must show as wrong bits, not as a fault)
    other = [rng.uniform(0.05, 0.95, L) for _ in range(6)]
    poison = dict(first0=other[0], first1=other[1], first2=other[2], X0=other[3], X1=other[4], X2=other[5])

    def call(T):
        h = C.c_void_p()
        raw(P, "fl_ibm_create", P.h, kind, L, ptr(T["first0"]), ptr(T["first1"]), ptr(T["first2"]), C.byref(h))
        T.release("first0", "first1", "first2")                 # copied into the set
        try:
            raw(P, "fl_ibm_update", h, ptr(T["X0"]), ptr(T["X1"]), ptr(T["X2"]))
            T.release("X0", "X1", "X2")
            raw(P, "fl_ibm_interp", h, 3, ptr(T["u"]), ptr(T["U"]))
            raw(P, "fl_ibm_spread", h, 3, ptr(T["F"]), ptr(T["dV"]), ptr(T["f"]))
            ab, force, torque = (C.c_double * 3)(*about), (C.c_double * 3)(), (C.c_double * 3)()
            raw(P, "fl_ibm_force", h, ptr(T["F"]), ptr(T["dV"]), None, 1, ab, force, torque)
            P.synchronize()
        finally:
            capi.lib.fl_ibm_destroy(h)
        return {"force": np.array(force[:]), "torque": np.array(torque[:])}

    def verify(res, what):
        assert np.allclose(res["U"].reshape(3, L), wantU, rtol=1e-12, atol=1e-13), what
        assert np.allclose(res["f"].reshape(3, -1), wantf, rtol=1e-12, atol=1e-12 * abs(wantf).max()), what
        assert fr.within(ref, "force", res["force"]) <= 1.0 and fr.within(ref, "torque", res["torque"]) <= 1.0, what
        assert np.array_equal(res["force"], ref["force"][0]) and np.array_equal(res["torque"], ref["torque"][0]), what
    try:
        drive(f"{gname} fl_ibm_create / update / interp / spread / force kind {kind}", spec, inputs, call, ["U", "f"], verify=verify, nx=n[0], P=P,
              fns=["fl_ibm_create", "fl_ibm_update", "fl_ibm_interp", "fl_ibm_spread", "fl_ibm_force", "fl_poisson_synchronize", "fl_ibm_destroy"], poison=poison)
    finally:
        P.close()


@pytest.mark.parametrize("angle", [0.0, 1e-9, math.pi / 2, 3.0], ids=["0", "1e-9", "pi/2", "3"])
def test_ibm_rigid_pose(ctx, angle):
    """fl_ibm_rigid_pose on 301 markers (two blocks of 256, the second partial): positions and target velocities against Rodrigues' rotation and
    velocity + omega x r in long double (tests/ibm_reference.py::rigid_pose), per entry within the bound that function derives from the operation
    count; the call with the velocities alone (X, Y, Z absent) and with the positions alone gives the same bits."""
    from tests import ibm_reference as ir
    P = ctx("G2").P
    L = 301
    rng = np.random.default_rng(77)
    X0 = rng.uniform(0.1, 0.9, (3, L))
    axis = np.array([2.0, -1.0, 2.0]) / 3.0
    c0, c, vel, om = [0.5, 0.4375, 0.25], [0.53, 0.41, 0.27], [0.3, -0.2, 0.1], [1.5, -2.0, 0.75]
    rotvec = axis * angle
    wX, wU, bX, bU = ir.rigid_pose(X0, c0, c, rotvec, vel, om)
    vec = lambda a: (C.c_double * 3)(*a)
    spec = [("X0", L, "in"), ("Y0", L, "in"), ("Z0", L, "in"), ("X", L, "out"), ("Y", L, "out"), ("Z", L, "out"), ("Ut", 3 * L, "out")]
    inputs = dict(X0=X0[0], Y0=X0[1], Z0=X0[2])

    def pose(T, xyz=True, ut=True):
        raw(P, "fl_ibm_rigid_pose", P.h, L, ptr(T["X0"]), ptr(T["Y0"]), ptr(T["Z0"]), vec(c0), vec(c), vec(rotvec), vec(vel), vec(om),
            *[ptr(T[n]) if xyz else None for n in "XYZ"], ptr(T["Ut"]) if ut else None)

    def verify(res, what):
        if "X" in res:
            got = np.stack([res[n] for n in "XYZ"])
            q = ir.rigid_pose_within(got, wX, bX)
            print(f"{what}: positions, largest error / bound = {q:.3f}")
            assert q <= 1.0, (what, q)
            if angle == 0.0:
                assert float(np.abs(got - (X0 + (np.array(c) - np.array(c0))[:, None])).max()) <= 4 * 2.0 ** -53, what
        if "Ut" in res:
            q = ir.rigid_pose_within(res["Ut"].reshape(3, L), wU, bU)
            print(f"{what}: velocities, largest error / bound = {q:.3f}")
            assert q <= 1.0, (what, q)
    fns = ["fl_ibm_rigid_pose"]
    both = drive(f"fl_ibm_rigid_pose angle {angle}", spec, inputs, quiet(pose), ["X", "Y", "Z", "Ut"], verify=verify, nx=L, P=P, fns=fns)
    only_u = drive(f"fl_ibm_rigid_pose angle {angle}, velocities alone", spec, inputs, quiet(lambda T: pose(T, xyz=False)), ["Ut"], verify=verify, nx=L, P=P, fns=fns)
    only_x = drive(f"fl_ibm_rigid_pose angle {angle}, positions alone", spec, inputs, quiet(lambda T: pose(T, ut=False)), ["X", "Y", "Z"], verify=verify, nx=L, P=P, fns=fns)
    for tag in both:
        assert same_bits(only_u[tag]["Ut"], both[tag]["Ut"]) and all(same_bits(only_x[tag][n], both[tag][n]) for n in "XYZ"), tag


# ------------------------------------------------------------------------------------------------------------------ the passive scalar

GAMMA = 0.0125


@GN
def test_scalar(gname):
    """fl_scalar_rhs, fl_scalar_step (superbee, 3 stages, in place), fl_scalar_stats, fl_scalar_cfl and fl_scalar_boundary_flux; the face
    velocities the handle borrows stand in the arena as well.  Bounds: the derived ones of tests/test_gpu_scalar.py, tests/test_gpu_scalar_step.py
    and tests/test_gpu_scalar_flux.py (tests/scalar_reference.py, tests/buoyancy_reference.py in long double)."""
    from tests.test_gpu_scalar_flux import check_flux
    n, bcname = GRIDS[gname][0], SCALAR_BC[gname]
    Pz, S = sc.make_handles(n, True, bcname, limiter="superbee", gamma=GAMMA)
    kinds, vals = sc.BC_SETS[bcname]
    Pr = sref.Problem(sc.faces(n, True), kinds, vals, GAMMA, "superbee")
    V = sc.velocity(n, bcname)
    q = sc.source(n)
    phi = sc.phi_field(n, "random") * 0.5 + sc.phi_field(n, "step")
    N = phi.size
    nfs = [v.size for v in V]
    adv, dif = sref.cfl(Pr, V, 1.0)
    dt = 0.5 / (adv + dif)
    wantR, E, _ = sref.rhs(Pr, phi, V, q, np.longdouble, bounds=True, limiter="superbee")
    tolR = sc.rhs_slack(E)
    wantS, B = sref.step(Pr, phi, V, dt, 3, q, np.longdouble, bounds=True)
    tolS = np.asarray(B, dtype=np.float64) * (1 + 2.0 ** -10)
    wcfl = sref.cfl(Pr, V, dt, np.longdouble)
    wmn, wmx, wsm = sref.stats(Pr, phi, np.longdouble)
    nb = min(1024, -(-N // 256))
    depth = -(-N // (256 * nb)) + 6 + 2 + nb + 3
    mag = float((np.abs(phi) * sref.volumes(Pr)).sum())
    base = [("Vx", nfs[0], "in"), ("Vy", nfs[1], "in"), ("Vz", nfs[2], "in"), ("phi", N, "in"), ("q", N, "in")]
    inputs = dict(Vx=V[0], Vy=V[1], Vz=V[2], phi=phi, q=q)

    def velocity(T):
        S.set_velocity(T["Vx"], T["Vy"], T["Vz"])

    def rhs(T):
        velocity(T)
        S.rhs(T["phi"], T["q"], out=T["R"])
        got = S.stats(T["phi"])
        return {"stats": np.array(got), "cfl": np.array(S.cfl(dt)), "flux": S.boundary_flux(T["phi"])}

    def verify(res, what):
        err = np.abs(res["R"].reshape(phi.shape).astype(np.longdouble) - wantR).astype(np.float64)        # tests/test_gpu_scalar.py:58-65
        assert (err <= tolR).all(), (what, float((err / tolR).max()))
        mn, mx, sm = res["stats"]                               # tests/test_gpu_scalar.py:113-126
        assert (mn, mx) == (wmn, wmx), what
        assert abs(sm - wsm) <= depth * sref.U * mag * (1 + 2.0 ** -10), what
        for got, w, ops in zip(res["cfl"], wcfl, (6, 9)):
            assert abs(got - w) <= ops * sref.U * abs(w) * (1 + 2.0 ** -10), (what, got, w)
        check_flux(res["flux"], Pr, phi, V, what)               # tests/test_gpu_scalar_flux.py:52-62
    try:
        drive(f"{gname} fl_scalar_rhs / stats / cfl / boundary_flux", base + [("R", N, "out")], inputs, rhs, ["R"], verify=verify, nx=n[0], P=Pz,
              fns=["fl_scalar_set_velocity", "fl_scalar_rhs", "fl_scalar_stats", "fl_scalar_cfl", "fl_scalar_boundary_flux"])
        spec = [("Vx", nfs[0], "in"), ("Vy", nfs[1], "in"), ("Vz", nfs[2], "in"), ("phi", N, "inout"), ("q", N, "in")]

        def step(T):
            velocity(T)
            S.step(T["phi"], dt, 3, T["q"])

        def verify_step(res, what):                             # tests/test_gpu_scalar_step.py:59-64
            got = res["phi"].reshape(phi.shape)
            err = np.abs(got.astype(np.longdouble) - wantS).astype(np.float64)
            assert (err <= tolS).all(), (what, float((err / tolS).max()))
            assert float(np.abs(got - phi).max()) > 1e-3, what
        drive(f"{gname} fl_scalar_step", spec, inputs, step, ["phi"], verify=verify_step, nx=n[0], P=Pz, fns=["fl_scalar_set_velocity", "fl_scalar_step"])

        def rhs_alone(T):                                       # the launches alone: nothing in the case waits
            velocity(T)
            S.rhs(T["phi"], T["q"], out=T["R"])
        drive(f"{gname} fl_scalar_rhs alone", base + [("R", N, "out")], inputs, rhs_alone, ["R"], placements=("A",), nx=n[0], P=Pz,
              fns=["fl_scalar_set_velocity", "fl_scalar_rhs"])
    finally:
        S.close()
        Pz.close()


# ------------------------------------------------------------------------------------------------------------------ several ranks

class RankCase:
    """G2 on a rank grid, in the form the handle helpers of tests/test_gpu_config5.py read"""

    def __init__(self, ranks):
        self.n, self.bc = GRIDS["G2"]
        self.ranks, self.box, self.kappa, self.own = ranks, CAVITY_BOX, 1e-3, None
        n = self.n
        self.size = ranks[0] * ranks[1] * ranks[2]
        self.xf = [np.linspace(CAVITY_BOX[d][0], CAVITY_BOX[d][1], n[d] + 1) for d in range(3)]
        self.g = g = fo.Grid(n, self.xf, self.bc, self.kappa)
        self.S = g.assemble_S()
        self.nullspace = True
        self.periodic = [False, False, False]
        self.shp = (n[2], n[1], n[0])
        self.fshape = [(n[2], n[1], g.nf[0]), (n[2], g.nf[1], n[0]), (g.nf[2], n[1], n[0])]


def _rank_flow_worker(R, case, ref):
    from tests.test_gpu_config5 import _blk, _fblk, _handle
    P, d, s = _handle(R, case)
    nx = int(d.len[0])
    seen = {}
    with torch.cuda.stream(s):
        p = _blk(case, d, ref["p"])
        vs = [_blk(case, d, ref["v"][a]) for a in range(3)]
        Vf = [_fblk(case, d, ref["V"][a], a) for a in range(3)]
        assert tuple(P.nface) == tuple(a.size for a in Vf)
        want = {**{f"V{a}": _fblk(case, d, ref["V-Gst"][a], a) for a in range(3)}, **{f"v{a}": _blk(case, d, ref["v-G"][a]) for a in range(3)}}
        N = p.size
        spec = [("p", N, "in")] + [(f"v{a}", N, "inout") for a in range(3)] + [(f"V{a}", Vf[a].size, "inout") for a in range(3)]
        inputs = {"p": p, **{f"v{a}": vs[a] for a in range(3)}, **{f"V{a}": Vf[a] for a in range(3)}}
        run_project(f"G2 {case.ranks} rank {R.rank} fl_poisson_project", P, nx, spec, inputs, set(PROJ[1:]), ABD, [], True, want, seen)
        b = _blk(case, d, ref["b"])

        def call(T):
            _, info = P.solve(T["b"], x=T["x"], history=True, **ref["kw"])
            return solve_extras(info)
        runs = drive(f"G2 {case.ranks} rank {R.rank} fl_poisson_solve", [("b", N, "in"), ("x", N, "out")], {"b": b}, call, ["x"], nx=nx, P=P, fns=["fl_poisson_solve"], ranks=True)
    P.close()
    return {"solve": runs, "paths": seen}


@pytest.mark.parametrize("ranks", [(2, 1, 1), (1, 1, 2)], ids=["2x1x1", "1x1x2"])
def test_ranks_project_and_cg(ranks):
    """G2 on two ranks, both in this process (tests/inproc.py): the blocks' projection takes k_project_six on the padded p where aligned and
    k_project_all elsewhere; k_cg_init and k_cg_finish touch the caller's b and x.  The gathered x of every placement against the oracle on the
    undecomposed grid, as _check_solve holds it."""
    from tests import mp_common as mpc
    from fluca_amd import capi
    case = RankCase(ranks)
    g, S = case.g, case.S
    p, vs, Vf, want = project_fields(g)
    _, b = mean_free_rhs(S, g.ncell)
    rtol = 1e-5
    xo, io = S.solve(b, ksp=fo.KSP_CG, pc=fo.PC_JACOBI, norm=fo.NORM_PRECONDITIONED, nullspace=True, rtol=rtol, maxit=10000)
    ref = dict(p=p, v=vs, V=Vf, b=b, kw=dict(type=0, pc=fo.PC_JACOBI, norm_type=fo.NORM_PRECONDITIONED, remove_nullspace=1, rtol=rtol, maxit=10000, check_every=7))
    ref["V-Gst"] = [want[f"V{a}"] for a in range(3)]
    ref["v-G"] = [want[f"v{a}"] for a in range(3)]
    out = inproc.run_threads(case.size, _rank_flow_worker, case, ref)
    paths = set()
    for o in out:
        paths |= set(o["paths"])
        assert SIX_PADDED in o["paths"] and SIX_DIRECT not in o["paths"], o["paths"]
    assert ALL_SINGLE in paths, paths

    class G:                    # what check_cg reads
        nullspace = True
    G.S = S
    for tag in out[0]["solve"]:
        x = np.full(case.shp, np.nan)
        for r in range(case.size):
            sl = mpc.block(mpc.decomp_of(capi, case.n, case.ranks, r))
            x[sl] = out[r]["solve"][tag]["x"].reshape(x[sl].shape)
        res = dict(out[0]["solve"][tag], x=x.ravel())
        for r in range(1, case.size):       # the statistics are collective
            assert out[r]["solve"][tag]["iters"] == res["iters"] and same_bits(out[r]["solve"][tag]["history"], res["history"])
        check_cg(G, b, xo, io, res, rtol, f"G2 {ranks} gathered [{tag}]")


def _rank_scalar_worker(R, case, blocks):
    from fluca_amd.scalar import Scalar
    from tests.test_gpu_config5 import _handle
    P, d, s = _handle(R, case)
    with torch.cuda.stream(s):
        S = Scalar(P, case.kinds, case.vals, limiter="superbee", gamma=GAMMA)
        Vb = [np.ascontiguousarray(blocks["V"][a][R.rank]).ravel() for a in range(3)]
        phi, q = blocks["phi"][R.rank].ravel(), blocks["q"][R.rank].ravel()
        N = phi.size
        assert tuple(P.nface) == tuple(v.size for v in Vb) and P.ncell == N
        spec = [("Vx", Vb[0].size, "in"), ("Vy", Vb[1].size, "in"), ("Vz", Vb[2].size, "in"), ("phi", N, "in"), ("q", N, "in"), ("R", N, "out")]

        def call(T):
            S.set_velocity(T["Vx"], T["Vy"], T["Vz"])
            S.rhs(T["phi"], T["q"], out=T["R"])
            s.synchronize()
        runs = drive(f"G2 {case.ranks} rank {R.rank} fl_scalar_rhs", spec, dict(Vx=Vb[0], Vy=Vb[1], Vz=Vb[2], phi=phi, q=q), call, ["R"], nx=int(d.len[0]),
                     P=P, fns=["fl_scalar_set_velocity", "fl_scalar_rhs"], ranks=True)
        S.close()
    P.close()
    return {tag: res["R"] for tag, res in runs.items()}


@pytest.mark.parametrize("ranks", [(2, 1, 1), (1, 1, 2)], ids=["2x1x1", "1x1x2"])
def test_ranks_scalar_rhs(ranks):
    """the ring kernels pack their slabs from the caller's phi; the gathered R of every placement against tests/scalar_reference.py on the global
    grid at the derived bound of tests/test_gpu_scalar_ranks.py::check_against_reference"""
    n = GRIDS["G2"][0]
    case = rk.Case(n, ranks, "neumann", uniform=True)
    V = sc.velocity(n, "neumann")
    phi, q = sc.phi_field(n, "random"), sc.source(n)
    blocks = {"V": [rk.scatter_faces(case, V[a], a) for a in range(3)], "q": rk.scatter_cells(case, q), "phi": rk.scatter_cells(case, phi)}
    res = inproc.run_threads(case.size, _rank_scalar_worker, case, blocks)
    kinds, vals = sc.BC_SETS["neumann"]
    Pr = sref.Problem(sc.faces(n, True), kinds, vals, GAMMA, "superbee")
    want, E, _ = sref.rhs(Pr, phi, V, q, np.longdouble, bounds=True, limiter="superbee")
    tol = sc.rhs_slack(E)
    for tag in res[0]:
        got = rk.gather_cells(case, [res[r][tag] for r in range(case.size)])
        err = np.abs(got.astype(np.longdouble) - want).astype(np.float64)
        print(f"G2 {ranks} fl_scalar_rhs gathered [{tag}]: largest error / bound = {float((err / tol).max()):.3f}")
        assert (err <= tol).all(), (tag, float((err / tol).max()))
