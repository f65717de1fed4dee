"""Passive scalar transport on top of the C-ABI (fl_scalar_*, include/fluca_hip.h): the right-hand side of the reference's transport
equation -- second-order TVD convection with its eleven limiters, two-point diffusion, a source -- and the s-stage second-order SSP
Runge-Kutta step of its tutorials (-ts_type ssp), one kernel launch per stage.  On a Poisson handle that is one rank's block of several
(fl_scalar_create_ranks) the arrays are that block, construction and rhs / step / cfl / stats are collective, and two layers of phi cross
every rank face once per stage.
"""
import ctypes as C
import weakref

import torch

from . import capi
from .capi import check, lib
from .poisson import _ptr

DIRICHLET, NEUMANN, PERIODIC = capi.SCALAR_DIRICHLET, capi.SCALAR_NEUMANN, capi.SCALAR_PERIODIC
LIMITERS = capi.LIMITERS


def limiter_from_name(name):
    out = C.c_int(-1)
    check(lib.fl_limiter_from_name(name.encode(), C.byref(out)), f"fl_limiter_from_name({name!r})")
    return out.value


def limiter_eval(limiter, r):
    out = C.c_double()
    check(lib.fl_limiter_eval(int(limiter), float(r), C.byref(out)), "fl_limiter_eval")
    return out.value


class Scalar:
    """bc: six kinds (DIRICHLET / NEUMANN / PERIODIC) in the order of the grid's boundaries; values: the six boundary values (a Neumann value is
    the derivative along the +axis).  The Poisson handle lends its grid, device and stream and must outlive this one."""

    def __init__(self, poisson, bc, values=None, limiter="superbee", gamma=0.0):
        self.P = poisson
        self.bc = tuple(int(b) for b in bc)
        h = C.c_void_p()
        # one rank's block of several: the collective constructor
        d = poisson.decomp
        several = d is not None and d.ranks[0] * d.ranks[1] * d.ranks[2] > 1
        create, name = (lib.fl_scalar_create_ranks, "fl_scalar_create_ranks") if several else (lib.fl_scalar_create, "fl_scalar_create")
        check(create(poisson.h, (C.c_int * 6)(*self.bc), C.byref(h)), name)
        self.h = h
        self.several = several
        poisson._children.append(weakref.ref(self))
        self._V = None
        for b, v in enumerate(values or ()):
            self.set_boundary_value(b, v)
        self.set_limiter(limiter)
        self.set_diffusivity(gamma)

    def close(self):
        if getattr(self, "h", None):
            lib.fl_scalar_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_boundary_value(self, boundary, value):
        check(lib.fl_scalar_set_boundary_value(self.h, int(boundary), float(value)), "fl_scalar_set_boundary_value")

    def set_limiter(self, limiter):
        self.limiter = limiter_from_name(limiter) if isinstance(limiter, str) else int(limiter)
        check(lib.fl_scalar_set_limiter(self.h, self.limiter), "fl_scalar_set_limiter")

    def set_diffusivity(self, gamma):
        check(lib.fl_scalar_set_diffusivity(self.h, float(gamma)), "fl_scalar_set_diffusivity")

    def set_velocity(self, Vx, Vy, Vz):
        """face velocities in the layouts of Poisson.rhs; borrowed (kept alive here) until the next call"""
        for t, n in zip((Vx, Vy, Vz), self.P.nface):
            assert t.numel() == n, "face array of the wrong length"
        self._V = (Vx, Vy, Vz)
        check(lib.fl_scalar_set_velocity(self.h, _ptr(Vx), _ptr(Vy), _ptr(Vz)), "fl_scalar_set_velocity")

    def rhs(self, phi, source=None, out=None):
        assert phi.numel() == self.P.ncell and (source is None or source.numel() == self.P.ncell)
        out = self.P.empty() if out is None else out
        self.P._pre()
        check(lib.fl_scalar_rhs(self.h, _ptr(phi), _ptr(source), _ptr(out)), "fl_scalar_rhs")
        self.P._post()
        return out

    def step(self, phi, dt, nstages=5, source=None):
        """advance phi in place over dt"""
        assert phi.numel() == self.P.ncell and (source is None or source.numel() == self.P.ncell)
        self.P._pre()
        check(lib.fl_scalar_step(self.h, float(dt), int(nstages), _ptr(source), _ptr(phi)), "fl_scalar_step")
        self.P._post()
        return phi

    def cfl(self, dt):
        """-> (convective, diffusive) Courant numbers of a step dt"""
        out = (C.c_double * 2)()
        self.P._pre()
        check(lib.fl_scalar_cfl(self.h, float(dt), out), "fl_scalar_cfl")
        self.P._post()
        return out[0], out[1]

    def stats(self, phi):
        """-> (min, max, sum phi vol)"""
        assert phi.numel() == self.P.ncell
        out = (C.c_double * 3)()
        self.P._pre()
        check(lib.fl_scalar_stats(self.h, _ptr(phi), out), "fl_scalar_stats")
        self.P._post()
        return out[0], out[1], out[2]

    def boundary_flux(self, phi):
        """-> (6, 2) array: per boundary the convective flux sum V phi_f A and the diffusive flux sum -Gamma g A through it, both along the +axis
        (fl_scalar_boundary_flux); a periodic end gives 0, 0"""
        import numpy as np
        assert phi.numel() == self.P.ncell
        out = (C.c_double * 12)()
        self.P._pre()
        check(lib.fl_scalar_boundary_flux(self.h, _ptr(phi), out), "fl_scalar_boundary_flux")
        self.P._post()
        return np.array(list(out), dtype=np.float64).reshape(6, 2)

    # ---- implicit diffusion (include/fluca_hip_implicit.h); on a handle of the collective constructor apply, solve and step_imex are the collective
    # calls of include/fluca_hip_implicit_ranks.h (one plane of phi across every rank face per Chebyshev step; the gathered result has the one-rank
    # bits).  `info` of a call: dict(steps, capped, emin, emax, bound), host values, the same on every rank

    def _implicit(self, name):
        name += "_ranks" if self.several else ""
        return getattr(lib, name), name

    @staticmethod
    def _info(i):
        return dict(steps=i.steps, capped=bool(i.capped), emin=i.emin, emax=i.emax, bound=i.bound)

    def diffusion_interval(self, c):
        """-> (emin, emax) of diag^-1 (I - c L): host arithmetic, no GPU work"""
        lo, hi = C.c_double(), C.c_double()
        check(lib.fl_scalar_diffusion_interval(self.h, float(c), C.byref(lo), C.byref(hi)), "fl_scalar_diffusion_interval")
        return lo.value, hi.value

    def diffusion_apply(self, c, phi, out=None):
        """out = phi - c D(phi); enqueues and returns"""
        assert phi.numel() == self.P.ncell
        out = self.P.empty() if out is None else out
        self.P._pre()
        f, name = self._implicit("fl_scalar_diffusion_apply")
        check(f(self.h, float(c), _ptr(phi), _ptr(out)), name)
        self.P._post()
        return out

    def diffusion_solve(self, c, b, x, rtol=1e-6, maxit=10000):
        """solve x - c D(x) = b in place in x (the guess) by Chebyshev-Jacobi, rtol relative to the initial error; -> info.  Enqueues and returns"""
        assert b.numel() == self.P.ncell and x.numel() == self.P.ncell
        info = capi.fl_scalar_cheb_info()
        self.P._pre()
        f, name = self._implicit("fl_scalar_diffusion_solve")
        check(f(self.h, float(c), float(rtol), int(maxit), _ptr(b), _ptr(x), C.byref(info)), name)
        self.P._post()
        return self._info(info)

    def step_imex(self, phi, dt, nstages=5, theta=1.0, rtol=1e-6, maxit=10000, source=None):
        """advance phi in place over dt: convection and source by the explicit stages, diffusion implicitly (theta = 1 backward Euler, 0.5
        Crank-Nicolson); -> info.  Enqueues and returns"""
        assert phi.numel() == self.P.ncell and (source is None or source.numel() == self.P.ncell)
        info = capi.fl_scalar_cheb_info()
        self.P._pre()
        f, name = self._implicit("fl_scalar_step_imex")
        check(f(self.h, float(dt), int(nstages), float(theta), float(rtol), int(maxit), _ptr(source), _ptr(phi), C.byref(info)), name)
        self.P._post()
        return self._info(info)
