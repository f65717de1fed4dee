/* fluca_hip_implicit_ranks.h -- the implicit scalar diffusion of fluca_hip_implicit.h (included below) on a rank's block of several: the Helmholtz
 * operator, its Chebyshev-Jacobi solve and the IMEX step as COLLECTIVE calls on a handle of fl_scalar_create_ranks over a decomposed grid.  An addition:
 * FL_ABI_VERSION does not change, no struct does, and the three names of fluca_hip_implicit.h keep refusing such a handle with FL_ERR_SUP.
 *
 * Every rank calls with the same c, dt, nstages, theta, rtol and maxit, as for fl_scalar_step on such a handle: nothing is voted.  The interval is host
 * arithmetic on the GLOBAL 1-D tables, so every rank gets the one-rank interval and the one-rank step count, and no call below reduces anything: no
 * all-reduce.  The 7-point star reaches one cell across a rank face: one exchange ships ONE plane of doubles across every boundary of the block
 * with a neighbouring rank (a periodic axis split over two ranks: both planes to the same peer), through the slabs of fl_scalar_step on the same
 * handle.  A cell runs the operations of the one-rank kernel on the same operands: gathered over the ranks, every result below has the bits of the
 * one-rank call of fluca_hip_implicit.h on the global grid, on every rank grid; info is the one-rank info on every rank.
 *
 * Stream order: everything a call does, its exchanges included, is ordered on the handle's stream; host arrays (info) are written before it
 * returns.  The host waits where fl_scalar_step waits on the same handle and nowhere else: RCCL transport -- not at all, the calls enqueue and
 * return; host-staged transport (fl_poisson_comm_init_host) -- once per exchange, for the planes to reach the host.
 *
 * On a one-rank handle each call IS the call of fluca_hip_implicit.h without the suffix: the same bits, the same launches. */
#ifndef FLUCA_HIP_IMPLICIT_RANKS_H
#define FLUCA_HIP_IMPLICIT_RANKS_H

#include "fluca_hip_implicit.h"

#ifdef __cplusplus
extern "C" {
#endif

/* fl_scalar_diffusion_apply: out = H_c(phi) on the rank's block; a rank face is no boundary (the handle's boundary values apply at the physical
 * boundaries of the block alone).  phi_dev, out_dev: the block's cells, CONSUMED; out_dev must not be phi_dev (FL_ERR_ARG_WRONG).  The argument
 * errors of fl_scalar_diffusion_apply, on every rank alike.  Wire: 1 exchange (one launch packs the planes, one launch applies). */
int fl_scalar_diffusion_apply_ranks(fl_scalar *m, double c, const double *phi_dev, double *out_dev);

/* fl_scalar_diffusion_solve: k = fl_scalar_cheb_steps(interval, rtol, maxit) steps, each one exchange and one launch; every step but the last stores
 * the planes the next exchange ships while it writes the iterate (no pack launch between two steps; one packs the guess).
 *   x_dev   the block's cells, CONSUMED: the initial guess in, the iterate out
 *   b_dev   the block's cells, CONSUMED; must not be x_dev (FL_ERR_ARG_WRONG)
 *   info    may be NULL; the same numbers on every rank
 * Wire: k exchanges, no all-reduce.  c = 0 or S = 0: one copy, no exchange, steps = 0.  The argument errors of fl_scalar_diffusion_solve. */
int fl_scalar_diffusion_solve_ranks(fl_scalar *m, double c, double rtol, int maxit, const double *b_dev, double *x_dev, fl_scalar_cheb_info *info);

/* fl_scalar_step_imex, in place on the rank's block: the stages of fl_scalar_step on this handle with Gamma = 0 (the high faces of V once, two planes
 * of phi per stage), the last of which stores the planes of phi* for the first Chebyshev step; then the k steps as above.
 *   source_dev  the block's cells or NULL, CONSUMED        phi_dev  the block's cells, CONSUMED: phi^n in, phi^{n+1} out        info  may be NULL
 * Wire: that of fl_scalar_step(dt, nstages) on this handle, + k exchanges; theta < 1: + 1 exchange (phi^n, for D(phi^n)).  Gamma = 0: exactly
 * fl_scalar_step on this handle, launch for launch and message for message.  The argument errors and FL_ERR_ARG_WRONGSTATE of fl_scalar_step_imex. */
int fl_scalar_step_imex_ranks(fl_scalar *m, double dt, int nstages, double theta, double rtol, int maxit, const double *source_dev, double *phi_dev,
                              fl_scalar_cheb_info *info);

#ifdef __cplusplus
}
#endif
#endif
