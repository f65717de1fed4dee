/* fluca_hip_implicit.h -- implicit diffusion of the passive scalar: the Helmholtz operator H_c = I - c D of the scalar's two-point diffusion term,
 * its solve by Chebyshev-Jacobi on a Gershgorin interval, and the IMEX step built on both.  An addition to fluca_hip.h (included below), which
 * declares fl_scalar and the error classes; FL_ABI_VERSION does not change, no struct of fluca_hip.h does.
 *
 * D(phi)(c) = sum_d [ g_d(f+) - g_d(f-) ] / h_d(c) with the two-point face gradient g and the boundary rule of fl_scalar_rhs (Dirichlet:
 * (phi_0 - phi_b) / (xc_0 - xf_0), mirrored at the high end; Neumann: the value, along the +axis; periodic: wrap) -- fl_scalar_rhs with V = 0,
 * Gamma = 1, q = 0.  D is affine in phi: D(phi) = L phi + d_bc.  With W = diag(cell volume), W (I - c L) is symmetric positive definite.
 *
 * The interval.  omega_d(i): the sum of the magnitudes of the off-diagonal entries of row i of axis d of L (only faces with a cell on the other
 * side, interior or periodic); S = c sum_d max_i omega_d(i).  I - c L is strictly diagonally dominant with a diagonal >= 1, so by Gershgorin the
 * spectrum of diag^-1 (I - c L) is real and lies in [emin, emax] = [1 / (1 + S), (1 + 2 S) / (1 + S)]: kappa = 1 + 2 S.  k Chebyshev steps on it
 * reduce the error, in the norm |e|^2 = sum_c vol_c diag_c e_c^2, by B_k = 2 s^k / (1 + s^2k), s = (sqrt kappa - 1) / (sqrt kappa + 1).
 * All of this is host arithmetic on the handle's 1-D tables, so the number of steps is known before the first launch and NOTHING on this path
 * looks at a norm: every call below that touches the GPU enqueues its launches on the handle's stream and returns.
 *
 * One rank only: on a handle of fl_scalar_create_ranks over a decomposed grid apply, solve and step_imex return FL_ERR_SUP (every rank holds such a
 * handle, so every rank returns it and nobody waits).  The collective calls for such a handle are fluca_hip_implicit_ranks.h's. */
#ifndef FLUCA_HIP_IMPLICIT_H
#define FLUCA_HIP_IMPLICIT_H

#include "fluca_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* What a solve ran: host values, filled before the call returns.  steps: Chebyshev steps enqueued (even; 0: x = b); capped: 1 if maxit cut the count
 * short of rtol; [emin, emax]: the interval; bound: B_steps, the guaranteed reduction of the initial error in the norm above (1 with 0 steps). */
typedef struct {
  int    steps, capped;
  double emin, emax, bound;
} fl_scalar_cheb_info;

/* Host only: the smallest EVEN k with B_k <= rtol on [emin, emax] (even: the iterate alternates between two arrays and ends in the caller's),
 * capped at maxit rounded down to even; *bound = B_k of the k returned.  FL_ERR_ARG_NULL: steps or bound missing; FL_ERR_ARG_OUTOFRANGE: rtol outside
 * (0, 1), maxit < 0, not 0 < emin <= emax, anything non-finite. */
int fl_scalar_cheb_steps(double emin, double emax, double rtol, int maxit, int *steps, double *bound);

/* [emin, emax] of diag^-1 (I - c L) as above.  Host arithmetic on the handle's tables: no GPU work.  c >= 0, finite (else FL_ERR_ARG_OUTOFRANGE);
 * c = 0, or a grid without a face between two cells: [1, 1]. */
int fl_scalar_diffusion_interval(fl_scalar *m, double c, double *emin, double *emax);

/* out = H_c(phi) = phi - c D(phi), the boundary values of the handle included.  phi_dev, out_dev: cells, CONSUMED (read / written in the call's stream
 * position); out_dev must not be phi_dev (FL_ERR_ARG_WRONG: neighbours still read phi).  c >= 0, finite.  One launch, 16 B/cell.  Enqueues and returns. */
int fl_scalar_diffusion_apply(fl_scalar *m, double c, const double *phi_dev, double *out_dev);

/* Solve H_c(x) = b by Chebyshev-Jacobi: fl_scalar_cheb_steps(interval, rtol, maxit) steps, one launch of 40 B/cell each (the first 32).
 *   x_dev   cells, CONSUMED: the initial guess in, the iterate out
 *   b_dev   cells, CONSUMED (read by every step; not written); must not be x_dev (FL_ERR_ARG_WRONG)
 *   rtol    in (0, 1), relative to the INITIAL ERROR x_guess - x in the norm above (not to a residual, not to b)
 *   maxit   >= 0; rounded down to even
 *   info    may be NULL
 * c = 0 or S = 0: no kernel, x gets b's bits by one copy, steps = 0.  No norm is formed and the host waits for nothing: enqueues and returns (the
 * first implicit call on a handle allocates its work arrays). */
int fl_scalar_diffusion_solve(fl_scalar *m, double c, double rtol, int maxit, const double *b_dev, double *x_dev, fl_scalar_cheb_info *info);

/* One IMEX step over dt, in place: convection and the source explicitly, diffusion implicitly.
 *   1. phi* = the step of fl_scalar_step(dt, nstages) with the diffusion term left out (its stage kernels run with Gamma = 0)
 *   2. b = phi* + (1 - theta) dt Gamma D(phi^n)
 *   3. H_{theta dt Gamma}(phi^{n+1}) = b, solved as fl_scalar_diffusion_solve does from the guess phi*
 * theta in [0.5, 1]: 1 is backward Euler -- b IS phi*, and nothing runs beside the nstages stage launches and the Chebyshev launches; 0.5 is
 * Crank-Nicolson (two more passes form b).  Gamma = 0: exactly fl_scalar_step, bit for bit, nothing else launched, steps = 0.
 *   source_dev  cells or NULL, CONSUMED        phi_dev  cells, CONSUMED: phi^n in, phi^{n+1} out        info  may be NULL
 * dt >= 0 finite, nstages >= 2, rtol in (0, 1), maxit >= 0 (else FL_ERR_ARG_OUTOFRANGE); FL_ERR_ARG_WRONGSTATE before a velocity is set (the arrays
 * of fl_scalar_set_velocity are read when the stage kernels run).  Enqueues and returns. */
int fl_scalar_step_imex(fl_scalar *m, double dt, int nstages, double theta, double rtol, int maxit, const double *source_dev, double *phi_dev,
                        fl_scalar_cheb_info *info);

#ifdef __cplusplus
}
#endif
#endif
