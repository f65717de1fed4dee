"""-m gpu: a handle's history changes no result, bit for bit (the catalogue, the state model and the walk: tests/handle_history.py).

One stretched 24 x 20 x 16 cavity grid (null space and its mean removal on, k_mom3 because ny > 8, three multigrid levels that end in
k_mg_coarse_cg).  One LIVE set of handles -- a Poisson, two Momentum and two Scalar handles on it, one set of markers -- runs a closed walk that
holds every ordered pair of operations once.  The first result of a (query, projection value) is kept, unless a fresh handle set has given one
already; every later one must equal it byte for byte.  Inputs are seeded host arrays, uploaded anew for every call into fresh device tensors,
so an in-place entry point never feeds its output back; outputs come back to the host before they are compared.

No operation is demoted: DEMOTED is empty.  An entry may be added only for an operation that test_two_fresh_handle_sets_agree shows not to be
reproducible run to run, with the tolerance of its existing reference test and the reason next to it.

What the first walks found: fl_poisson_solve with FL_KSP_CHEBYSHEV and FL_NORM_NONE returned as its history what earlier solves had left in the
handle's history buffer (zeros on a fresh handle, norms or a NaN later; fixed in fl_solve_cheb); and the last bit of fl_momentum_rhs follows the
kernel the momentum state selects (k_mom3 with v0, k_mom2 without), so the momentum profile is in its projection.

fl_poisson_set_stream: the caller synchronises the handle before it switches (include/fluca_hip.h); the stream setter here does."""
import ctypes as C
from collections import Counter

import numpy as np
import pytest

from tests import handle_history as hh
from tests import inproc

pytestmark = pytest.mark.gpu

N = (24, 20, 16)
KAPPA = 1e-3
SEEDS = hh.SEEDS
RANK_SEED = hh.RANK_SEED
DEMOTED = {}            # operation -> (rtol, atol); see the docstring
EXPECTED = {}           # (query, projection value) -> result of a fresh handle set in the default state (test_two_fresh_handle_sets_agree)

CG, BCGS, CHEB, GMRES = 0, 1, 2, 3
NONE, JACOBI, MG = 0, 1, 2
NORM_NONE = 3


# ------------------------------------------------------------------------------------------------------------------ seeded inputs, built once

class Inputs:
    def __init__(self):
        from oracle import fluca_oracle as fo
        from tests.gpu_common import CAVITY, CAVITY_BOX, stretched_faces
        from tests.test_gpu_ibm import sphere_markers
        n = N
        self.bc, self.xf = CAVITY, stretched_faces(n, CAVITY_BOX)
        g = self.g = fo.Grid(n, self.xf, CAVITY, KAPPA)
        self.shp = (n[2], n[1], n[0])
        self.fshape = [(n[2], n[1], g.nf[0]), (n[2], g.nf[1], n[0]), (g.nf[2], n[1], n[0])]
        self.periodic = [False, False, False]
        nc, nf = g.ncell, [int(v) for v in g.nface]
        rng = np.random.default_rng(20261020)
        cells = lambda k=None: rng.standard_normal(nc if k is None else (k, nc))
        faces = lambda s=1.0: [s * rng.standard_normal(nf[d]) for d in range(3)]
        p = rng.uniform(-1.0, 1.0, nc)
        p -= p.mean()
        self.b = g.assemble_S().mult(p)                       # in the range of the singular S
        self.bnan = self.b.copy()
        self.bnan[nc // 2 + 3] = np.nan                         # an interior cell, as the stop tests place it
        self.c = cells(6)
        self.Y = cells(10)                                      # more vectors than one launch of fl_vec_mdot takes (8)
        self.alpha = rng.standard_normal(10)
        self.F = faces()
        self.v = cells(3).ravel()
        self.v2 = cells(3).ravel()
        self.vbc9 = [rng.standard_normal(nf[q % 3]) for q in range(9)]
        self.plane = rng.standard_normal(n[1] * n[2])
        hmin = min(np.diff(self.xf[d]).min() for d in range(3))
        # the three momentum profiles
        dt2, rho2 = 0.4 * hmin, 1.3
        mu2 = 0.8 * rho2 * hmin * hmin / dt2
        self.mom = {
            "M1": dict(dt=KAPPA, rho=1.0, mu=0.05, V0=faces(), W=[rng.standard_normal(nf[q % 3]) for q in range(9)], v0=None),
            "M2": dict(dt=dt2, rho=rho2, mu=mu2, V0=faces(0.4), W=None, v0=0.4 * rng.uniform(-1, 1, 3 * nc)),
            "M3": dict(dt=dt2, rho=rho2, mu=mu2, V0=faces(0.3), W=None, v0=0.3 * rng.uniform(-1, 1, 3 * nc), coeff=(1.0, 0.5 * dt2, -0.5 * mu2 * dt2 / rho2)),
        }
        # the scalar: kinds, values, two sets of face velocities
        self.skinds = (0, 1, 0, 1, 1, 0)
        self.svals = (0.7, -0.4, 0.25, 1.5, -1.1, 0.6)
        self.Va, self.Vb = [], []
        for dst in (self.Va, self.Vb):
            for d in range(3):
                a = rng.uniform(-1.0, 1.0, nf[d])
                a[rng.uniform(size=nf[d]) < 0.1] = 0.0
                dst.append(a)
        self.phi = rng.uniform(-1.0, 1.0, nc)
        self.q = rng.uniform(-1.0, 1.0, nc)
        self.sdt = 0.1 * hmin
        # the markers: a sphere inside the cavity, and the same sphere moved and shrunk
        L = self.L = 61
        self.XA = sphere_markers(L, (0.5, 0.5, 0.25), 0.15)
        self.XB = sphere_markers(L, (0.45, 0.55, 0.22), 0.12)
        self.u = cells(3).ravel()
        self.Fm = rng.standard_normal(3 * L)
        self.dV = rng.uniform(0.5, 1.5, L) * 1e-3
        self.f0 = cells(3).ravel()
        self.phis = cells(2)


_INPUTS = None


def inputs():
    global _INPUTS
    if _INPUTS is None:
        _INPUTS = Inputs()
    return _INPUTS


class RankCase:
    """the grid on a rank grid, in the form the handle helper of tests/test_gpu_config5.py reads"""

    def __init__(self, inp, ranks):
        self.n, self.ranks, self.bc, self.xf, self.kappa, self.own = N, ranks, inp.bc, inp.xf, KAPPA, None
        self.shp, self.fshape, self.periodic = inp.shp, inp.fshape, inp.periodic


# ------------------------------------------------------------------------------------------------------------------ the handles

class HandleSet:
    """A Poisson, Momentum and Scalar handles on it and one marker set, in the default state of tests/handle_history.py.  R: this rank of an
    in-process rank grid (tests/inproc.py), None = the whole grid on one handle."""

    def __init__(self, ops, R=None, case=None):
        import torch
        from fluca_amd import capi
        from fluca_amd.poisson import Momentum, Poisson
        from fluca_amd.scalar import Scalar
        from tests.test_gpu_ibm import Ibm
        self.torch, self.capi, self.lib, self.check = torch, capi, capi.lib, capi.check
        self.inp = inp = inputs()
        self.R, self.case, self.ops = R, case, ops
        handles = {o.handle for o in ops}
        if R is None:
            self.P, self.d = Poisson(N, inp.xf, inp.bc, KAPPA), None
            self.check(self.lib.fl_poisson_set_stream(self.P.h, None))          # the handle's own stream
            self.own = None
        else:
            from tests.test_gpu_config5 import _handle
            self.P, self.d, self.own = _handle(R, case)
        self.P._ext_stream = True               # this file orders the streams itself: a host wait before and after every call
        self.second = torch.cuda.Stream()
        self.nM = 2 if "m1" in handles else 1
        self.nS = 2 if "s1" in handles else 1
        self.M = [Momentum(self.P) for _ in range(self.nM)]
        self.S = [Scalar(self.P, inp.skinds, inp.svals) for _ in range(self.nS)]
        self.keepV = [None] * self.nS
        self.knobs0 = {}
        for name in hh.ALT_KNOBS:
            v = C.c_int()
            self.check(self.lib.fl_tuning_get(name.encode(), C.byref(v)))
            self.knobs0[name] = v.value
        for i in range(self.nM):
            self.set_mom(i, "M1")
            self.set_ainv(i, "II")
        for i in range(self.nS):
            self.set_scalar(i, "S1")
        self.ready()
        self.ibm = Ibm(self.P, 0, [self.blockless(a) for a in inp.XA])
        self.done()

    # ---- blocks of the global arrays, transfers, the two host waits around every call
    def blockless(self, a):
        return np.ascontiguousarray(a, dtype=np.float64)

    def cell(self, a):
        if self.d is None:
            return a
        from tests.test_gpu_config5 import _blk
        return _blk(self.case, self.d, a)

    def cells(self, a, k=3):
        return np.concatenate([self.cell(c) for c in np.asarray(a).reshape(k, -1)])

    def face(self, a, ax):
        if self.d is None:
            return a
        from tests.test_gpu_config5 import _fblk
        return _fblk(self.case, self.d, a, ax)

    def up(self, a):
        return self.torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64).ravel(), device="cuda")

    def upc(self, a):
        return self.up(self.cell(a))

    def upf(self, three):
        return [self.up(self.face(three[d], d)) for d in range(3)]

    def ready(self):
        """the uploads have arrived"""
        self.torch.cuda.current_stream().synchronize()

    def done(self):
        """the handle's stream has run dry"""
        self.P.synchronize()

    def get(self, t):
        return t.cpu().numpy().copy()

    def close(self):
        self.done()
        self.ibm.close()
        self.P.close()

    # ---- setters
    def set_mom(self, i, prof):
        s, M = self.inp.mom[prof], self.M[i]
        V0 = self.upf(s["V0"])
        if s["v0"] is None:
            W = [self.up(self.face(s["W"][q], q % 3)) for q in range(9)]
            self.ready()
            M.set_state(s["dt"], s["rho"], s["mu"], V0, W)
        else:
            v0 = self.up(self.cells(s["v0"]))
            self.ready()
            W = M.interp_faces(v0)              # v0interp = B v0, as fl_momentum_set_state_v0 wants it
            M.set_state(s["dt"], s["rho"], s["mu"], V0, W, v0=v0)
        if "coeff" in s:
            M.set_coefficients(*s["coeff"])
        self.done()

    def set_ainv(self, i, prof):
        self.M[i].set_ainv_types(*{"II": (0, 0), "DD": (1, 1), "RI": (2, 0)}[prof])

    def set_scalar(self, i, prof):
        S, inp = self.S[i], self.inp
        limiter, gamma, vals, V = {"S1": ("superbee", 0.0, inp.svals, inp.Va), "S2": ("venkatakrishnan", 0.0125, inp.svals[:1] + (0.9,) + inp.svals[2:], inp.Va),
                                   "S3": ("upwind", 0.0125, inp.svals, inp.Vb)}[prof]
        S.set_limiter(limiter)
        S.set_diffusivity(gamma)
        for b, v in enumerate(vals):
            S.set_boundary_value(b, v)
        self.keepV[i] = self.upf(V)             # borrowed by the handle: new device arrays with every profile
        self.ready()
        S.set_velocity(*self.keepV[i])

    def set_knobs(self, prof):
        values = hh.ALT_KNOBS if prof == "alt" else self.knobs0
        if self.R is not None:                  # process-wide: every rank's thread sets the same value while nobody is inside a call
            self.R.barrier()
        for name, v in values.items():
            self.check(self.lib.fl_tuning_set(name.encode(), int(v)))
        if self.R is not None:
            self.R.barrier()

    def set_ibm(self, prof):
        X = self.inp.XA if prof == "A" else self.inp.XB
        self.ibm.Xd = [self.up(a) for a in X]
        self.ready()
        self.check(self.lib.fl_ibm_update(self.ibm.h, *[C.c_void_p(t.data_ptr()) for t in self.ibm.Xd]), "fl_ibm_update")
        self.done()

    def set_stream(self, which):
        """include/fluca_hip.h: fl_poisson_set_stream orders nothing; the caller waits for the handle before it switches"""
        self.done()
        s = self.own if which == "own" else self.second
        self.check(self.lib.fl_poisson_set_stream(self.P.h, None if s is None else C.c_void_p(s.cuda_stream)))

    def setter(self, op, state):
        (var, val), = op.sets.items()
        if var.startswith("mom"):
            self.set_mom(int(var[-1]), val)
        elif var.startswith("ainv"):
            self.set_ainv(int(var[-1]), val)
        elif var.startswith("sc"):
            self.set_scalar(int(var[-1]), val)
        else:
            {"knobs": self.set_knobs, "ibm": self.set_ibm, "stream": self.set_stream}[var](val)

    # ---- queries: name -> outputs
    def query(self, op, state):
        where, what = op.name.split(".", 1)
        fn = getattr(self, "q_" + {"p": "p", "m": "m", "s": "s", "i": "ibm"}[where[0]])
        out = fn(what) if where in ("p", "ibm") else fn(int(where[1]), what)
        return {k: (self.get(v) if hasattr(v, "is_cuda") else np.asarray(v)) for k, v in out.items()}

    def solve_out(self, x, info, tag=""):
        out = {tag + "x": self.get(x), tag + "reason": info["reason"], tag + "iters": info["iters"], tag + "rnorm0": info["rnorm0"], tag + "rnorm": info["rnorm"]}
        if "history" in info:
            out[tag + "history"] = np.asarray(info["history"])
        return out

    def psolve(self, b, tag="", **kw):
        bd = self.upc(b)
        self.ready()
        x, info = self.P.solve(bd, history=True, remove_nullspace=1, **kw)
        self.done()
        return self.solve_out(x, info, tag)

    def q_p(self, what):
        P, inp, lib, check = self.P, self.inp, self.lib, self.check
        ptr = lambda t: C.c_void_p(t.data_ptr())
        if what == "apply":
            x = self.upc(inp.c[0])
            self.ready()
            y = P.apply(x)
            self.done()
            return {"y": y}
        if what == "diagonal":
            d = P.diagonal()
            self.done()
            return {"d": d}
        if what == "rhs":
            V, cr = self.upf(inp.F), self.upc(inp.c[1])
            self.ready()
            b = P.rhs(*V, contrhs=cr)
            self.done()
            return {"b": b}
        if what == "project":
            p, v, V = self.upc(inp.c[2]), [self.upc(inp.c[3 + a]) for a in range(3)], self.upf(inp.F)
            self.ready()
            P.project(p, v=v, V=V)
            self.done()
            return {**{f"v{a}": v[a] for a in range(3)}, **{f"V{a}": V[a] for a in range(3)}}
        if what == "gst_bc":
            pb, V = self.up(inp.plane), self.up(inp.F[0])
            self.ready()
            P.gst_bc(1, pb, V)
            self.done()
            return {"V": V}
        if what == "pressure_update":
            out = {}
            for first in (1, 0):
                dp, p0, ph, p = [self.upc(inp.c[a]) for a in range(4)]
                self.ready()
                P.pressure_update(first, dp, p0, ph, p)
                self.done()
                out.update({f"phalf{first}": ph, f"p{first}": p})
            return out
        if what == "gershgorin":
            out = {}
            for pc in (NONE, JACOBI):
                v = C.c_double()
                check(lib.fl_poisson_gershgorin(P.h, pc, C.byref(v)))
                out[f"bound{pc}"] = v.value
            return out
        if what == "solve cg 12":
            return self.psolve(inp.b, type=CG, pc=JACOBI, maxit=12)
        if what == "solve cg rtol":
            return self.psolve(inp.b, type=CG, pc=JACOBI, rtol=1e-8, maxit=3000)
        if what == "solve cg single reduction 12":
            return self.psolve(inp.b, type=CG, pc=JACOBI, maxit=12, cg_single_reduction=1)
        if what == "solve bcgs 12":
            return self.psolve(inp.b, type=BCGS, pc=JACOBI, maxit=12)
        if what == "solve chebyshev 12":
            return self.psolve(inp.b, type=CHEB, pc=JACOBI, norm_type=NORM_NONE, maxit=12)
        if what.startswith("solve mg"):
            kw = {"solve mg levels 0": dict(mg_levels=0), "solve mg levels 2 smooth 2": dict(mg_levels=2, mg_smooth_its=2), "solve mg levels 1": dict(mg_levels=1)}[what]
            return self.psolve(inp.b, type=CG, pc=MG, rtol=1e-8, maxit=40, **kw)
        if what == "solve cg 600 history then short":
            out = self.psolve(inp.b, "long ", type=CG, pc=JACOBI, rtol=1e-13, maxit=600)
            out.update(self.psolve(inp.b, "short ", type=CG, pc=JACOBI, maxit=5))
            return out
        if what == "solve cg nan":
            out = self.psolve(inp.bnan, type=CG, pc=JACOBI, maxit=30)
            return {"reason": out["reason"], "iters": out["iters"]}
        n = P.ncell
        if what == "vec_lincomb":
            x, z, y = self.upc(inp.c[0]), self.upc(inp.c[1]), P.empty()
            self.ready()
            check(lib.fl_vec_lincomb(P.h, n, 0.75, ptr(x), -1.25, ptr(z), ptr(y)))
            self.done()
            return {"y": y}
        if what == "vec_dot":
            x, y, r = self.upc(inp.c[0]), self.upc(inp.c[1]), C.c_double()
            self.ready()
            check(lib.fl_vec_dot(P.h, n, ptr(x), ptr(y), C.byref(r)))
            self.done()
            return {"dot": r.value}
        k = len(inp.Y)
        x, ys = self.upc(inp.c[0]), [self.upc(a) for a in inp.Y]
        ptrs = (C.c_void_p * k)(*[t.data_ptr() for t in ys])
        self.ready()
        if what == "vec_mdot":
            out = (C.c_double * k)()
            check(lib.fl_vec_mdot(P.h, n, ptr(x), ptrs, k, out))
            self.done()
            return {"dots": np.array(out[:])}
        assert what == "vec_maxpy", what
        check(lib.fl_vec_maxpy(P.h, n, ptr(x), (C.c_double * k)(*inp.alpha), ptrs, k))
        self.done()
        return {"x": x}

    def msolve(self, M, guess=None, **kw):
        b = self.up(self.cells(self.inp.v2))
        x = None if guess is None else self.up(self.cells(guess))
        self.ready()
        x, info = M.solve(b, x=x, history=True, pc=JACOBI, **kw)
        self.done()
        return self.solve_out(x, info)

    def q_m(self, i, what):
        from fluca_amd.poisson import KspOptions
        M, P, inp = self.M[i], self.P, self.inp
        v = self.up(self.cells(inp.v))
        if what == "apply":
            self.ready()
            y = M.apply(v)
            self.done()
            return {"y": y}
        if what in ("diagonal", "rowsum"):
            d = getattr(M, what)()
            self.done()
            return {"d": d}
        if what == "gershgorin":
            return {"radius": M.gershgorin()}
        if what == "chebyshev_interval":
            return {"interval": np.array(M.chebyshev_interval())}
        if what == "solve bcgs":
            return self.msolve(M, type=BCGS, rtol=1e-8, maxit=200)
        if what == "solve gmres5":
            return self.msolve(M, type=GMRES, gmres_restart=5, rtol=1e-8, maxit=100)
        if what == "solve chebyshev":
            return self.msolve(M, type=CHEB, rtol=1e-8, maxit=200, check_every=5)
        if what == "solve chebyshev guess":
            return self.msolve(M, guess=0.5 * inp.v2 + 0.01 * inp.v, type=CHEB, rtol=1e-8, maxit=200, check_every=3, initial_guess_nonzero=1)
        if what == "face_interp":
            rhs = self.upf(inp.F)
            self.ready()
            V = M.face_interp(v, rhs)
            self.done()
            return {f"V{d}": V[d] for d in range(3)}
        if what == "interp_faces":
            vbc = [self.up(self.face(inp.vbc9[q], q % 3)) for q in range(9)]
            self.ready()
            W = M.interp_faces(v, vbc)
            self.done()
            return {f"W{q}": W[q] for q in range(9)}
        if what == "rhs":
            p, vbc = self.upc(inp.c[2]), self.up(self.cells(inp.v2))
            self.ready()
            out = M.rhs(0.013, 13.0, 0.4, v, p, vbc)
            self.done()
            return {"momrhs": out}
        if what == "add_buoyancy":
            phis = [self.upc(a) for a in inp.phis]
            self.ready()
            M.add_buoyancy(v, phis, [(0.0, -0.3, 0.0), (0.1, 0.0, 0.2)], [0.5, -0.25], 0.01)
            self.done()
            return {"momrhs": v}
        if what == "jacobian_mult":
            V, p = self.upf(inp.F), self.upc(inp.c[2])
            self.ready()
            fv, fV, fp = M.jacobian_mult(v, V, p)
            self.done()
            return {"fv": fv, "fp": fp, **{f"fV{d}": fV[d] for d in range(3)}}
        if what == "schur_apply":
            p = self.upc(inp.c[2])
            self.ready()
            y = M.schur_apply(p)
            self.done()
            return {"y": y}
        assert what == "abf_apply", what
        self.ready()
        vv, V, p, info = M.abf_apply(v, momentum=KspOptions(type=BCGS, rtol=1e-8, maxit=200), schur=KspOptions(rtol=1e-6, maxit=40, remove_nullspace=1))
        self.done()
        out = {"v": vv, "p": p, **{f"V{d}": V[d] for d in range(3)}}
        for j in range(2):
            out.update({f"iters{j}": info[j]["iters"], f"reason{j}": info[j]["reason"], f"rnorm{j}": info[j]["rnorm"]})
        return out

    def q_s(self, i, what):
        S, inp = self.S[i], self.inp
        phi, q = self.upc(inp.phi), self.upc(inp.q)
        self.ready()
        if what in ("rhs", "rhs source"):
            out = S.rhs(phi, q if what == "rhs source" else None)
            self.done()
            return {"R": out}
        if what.startswith("step"):
            S.step(phi, inp.sdt, int(what.split()[1]), q)
            self.done()
            return {"phi": phi}
        if what == "cfl":
            return {"cfl": np.array(S.cfl(inp.sdt))}
        if what == "stats":
            return {"stats": np.array(S.stats(phi))}
        assert what == "boundary_flux", what
        return {"flux": S.boundary_flux(phi)}

    def q_ibm(self, what):
        ibm, inp, L = self.ibm, self.inp, self.inp.L
        if what == "interp":
            u = self.up(self.cells(inp.u))
            self.ready()
            U = ibm.interp(u, 3)
            self.done()
            return {"U": U}
        F, dV = self.up(inp.Fm), self.up(inp.dV)
        if what == "spread":
            f = self.up(self.cells(inp.f0))
            self.ready()
            ibm.spread(F, dV, f, 3)
            self.done()
            return {"f": f}
        assert what == "force", what
        about, force, torque = (C.c_double * 3)(0.5, 0.4375, 0.25), (C.c_double * 3)(), (C.c_double * 3)()
        self.ready()
        self.check(self.lib.fl_ibm_force(ibm.h, C.c_void_p(F.data_ptr()), C.c_void_p(dV.data_ptr()), None, 1, about, force, torque), "fl_ibm_force")
        self.done()
        return {"force": np.array(force[:]), "torque": np.array(torque[:])}


# ------------------------------------------------------------------------------------------------------------------ one rank

OPS = hh.catalogue()
QUERIES = [o for o in OPS if o.kind == "query"]


@pytest.mark.parametrize("op", QUERIES, ids=[o.name.replace(" ", "_") for o in QUERIES])
def test_two_fresh_handle_sets_agree(op):
    """The determinism the walks rely on: the query on two handle sets created for it alone, in the default state -- the same bits.  The result
    seeds the table the walks compare with."""
    res = []
    for _ in range(2):
        H = HandleSet(OPS)
        try:
            res.append(H.query(op, hh.initial(OPS)))
        finally:
            H.close()
    d = hh.first_difference(res[0], res[1], DEMOTED.get(op.name))
    assert d is None, f"{op.name} on two fresh handle sets: output {d[0]!r} index {d[1]}: {d[2]!r} against {d[3]!r}"
    EXPECTED[(op.name, hh.projection(op, hh.initial(OPS)))] = res[0]
    # ... and one fresh set per other projection value the walks meet, put straight into it: a value that is wrong in the same way on every
    # visit of a walk (tests/handle_history.py: seed_expected) differs from this one

    def close(H):
        try:
            H.set_knobs("default")
        finally:
            H.close()
    hh.seed_expected(lambda: HandleSet(OPS), OPS, [hh.walk(OPS, s) for s in SEEDS], EXPECTED, only=op.name, close=close)


@pytest.mark.parametrize("seed", SEEDS)
def test_walk(seed):
    """The live set runs the whole circuit; a failure names the operation, its last three predecessors, the logical state, the output, the first
    index that differs and both values."""
    steps = hh.walk(OPS, seed)
    H = HandleSet(OPS)
    try:
        findings = hh.run(H, OPS, steps, dict(EXPECTED), DEMOTED)
    finally:
        try:
            H.set_knobs("default")              # the stream goes with the handle
        finally:
            H.close()
    print(sorted(Counter((f.op, f.output) for f in findings).items()))       # all of them in short, then the first twenty in full
    for f in findings[:20]:
        print(hh.describe(f))
    assert not findings, f"{len(findings)} results depend on the history; the first: {hh.describe(findings[0])}"


# ------------------------------------------------------------------------------------------------------------------ two ranks in one process

RANK_OPS = hh.rank_catalogue()


def _rank_worker(R, case, steps):
    import torch
    H = HandleSet(RANK_OPS, R, case)
    try:
        with torch.cuda.stream(H.own):
            findings = hh.run(H, RANK_OPS, steps, {}, DEMOTED)
    finally:
        H.set_knobs("default")
        H.close()
    print(f"rank {R.rank}:", sorted(Counter((f.op, f.output) for f in findings).items()))
    return [hh.describe(f) for f in findings]


def test_walk_on_two_ranks():
    """2 x 1 x 1 ranks, one thread and one handle set each, the SAME walk on both so that the collectives pair up; the catalogue is what is
    rank-specific (tests/handle_history.py: rank_catalogue).  Per rank: first occurrence kept, every later one equal."""
    from fluca_amd import capi
    case = RankCase(inputs(), (2, 1, 1))
    steps = hh.walk(RANK_OPS, RANK_SEED)
    before = {}
    for name in hh.ALT_KNOBS:
        v = C.c_int()
        capi.check(capi.lib.fl_tuning_get(name.encode(), C.byref(v)))
        before[name] = v.value
    try:
        res = inproc.run_threads(2, _rank_worker, case, steps)
    finally:
        for name, v in before.items():
            capi.check(capi.lib.fl_tuning_set(name.encode(), v))
    for r, found in enumerate(res):
        for line in found[:20]:
            print(f"rank {r}: {line}")
    assert not any(res), f"results depend on the history: rank 0 {len(res[0])}, rank 1 {len(res[1])}; the first: {(res[0] + res[1])[0]}"
