// fl_limiter.h -- the eleven flux limiters psi(r) of the second-order TVD face value (fluca/src/fd/impls/secondordertvd/secondordertvdlimiter.c),
// numbered in the reference's registration order.  One definition for the host (fl_limiter_eval) and for the kernel (fl_scalar.hip).
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FL_HD __host__ __device__ __forceinline__
#else
#define FL_HD inline
#endif

namespace fl {

enum Limiter {
  LIM_SUPERBEE = 0, LIM_MINMOD, LIM_MC, LIM_VANLEER, LIM_VANALBADA, LIM_BARTHJESPERSON, LIM_VENKATAKRISHNAN, LIM_KOREN, LIM_UPWIND, LIM_SOU, LIM_QUICK,
  LIM_COUNT
};

// (the reference's PetscMin / PetscMax: comparisons, not fmin / fmax)
FL_HD double lim_min(double a, double b) { return a < b ? a : b; }
FL_HD double lim_max(double a, double b) { return a < b ? b : a; }

template <int L>
FL_HD double limiter(double r)
{
  if (L == LIM_SUPERBEE) return lim_max(0., lim_max(lim_min(2. * r, 1.), lim_min(r, 2.)));
  if (L == LIM_MINMOD) return lim_max(0., lim_min(r, 1.));
  if (L == LIM_MC) return lim_max(0., lim_min(lim_min(2. * r, (1. + r) / 2.), 2.));
  if (L == LIM_VANLEER) {
    const double a = r < 0. ? -r : r;
    return (r + a) / (1. + a);
  }
  if (L == LIM_VANALBADA) return r <= 0. ? 0. : (r * r + r) / (r * r + 1.);
  if (L == LIM_BARTHJESPERSON) {
    if (r <= 0.) return 0.;
    const double a = 4. * r / (1. + r), b = 4. / (1. + r);
    return (1. + r) / 2. * lim_min(1., lim_min(a, b));
  }
  if (L == LIM_VENKATAKRISHNAN) {
    const double a = 4. * r * (3. * r + 1) / (11. * r * r + 4. * r + 1.), b = 4. * (r + 3.) / (r * r + 4. * r + 11.);
    return r <= 0. ? 0. : (1. + r) / 2. * lim_min(a, b);
  }
  if (L == LIM_KOREN) return lim_max(0., lim_min(lim_min(2. * r, (1. + 2. * r) / 3.), 2.));
  if (L == LIM_UPWIND) return 0.;
  if (L == LIM_SOU) return r;
  return (3. + r) / 4.;  // LIM_QUICK
}

}  // namespace fl
