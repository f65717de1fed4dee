// fl_mom_solve.hip -- KSPSolve(kspA): the Krylov drivers on the momentum operator of fl_momentum.hip.  Left-preconditioned BiCGStab (KSPBCGS), restarted
// GMRES (KSPGMRES, the reference's default type for kspA, abfpc.c:72) or Chebyshev (KSPCHEBYSHEV), PCJACOBI or PCNONE, from a zero or a given guess.
// Host control flow only: the products and vector updates are launched through fl_mom_handle.h, the Krylov scalars live in fl_ksp.hip.
#include "fl_gmres_lsq.h"
#include "fl_mom_handle.h"

using namespace fl;

// out = a ./ d
__global__ void __launch_bounds__(256) k_div(int64_t n, const double *__restrict__ a, const double *__restrict__ d, double *__restrict__ out)
{
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) out[i] = a[i] / d[i];
}

// KSPCHEBYSHEV on the momentum block (-ns_abf_momentum_ksp_type chebyshev, a PETSc option the reference's kspA accepts like any other):
// PETSc's three-term recurrence with PCJACOBI / PCNONE, zero initial guess.  Interval: opts->emin / emax (-ksp_chebyshev_eigenvalues), or, with
// PCJACOBI, fl_momentum_chebyshev_interval: [max(1 - g, 0.9 / mean a_ii), 1 + g], g the Gershgorin radius of D^-1 A -- a heuristic for emin, a bound for
// emax, and a REAL interval for a spectrum that is not (the convective part of g is imaginary): PETSc would have estimated the spectrum with GMRES.
// So a solve on the default interval is never left unwatched: with -ksp_norm_type none it still forms the preconditioned norm and stops with
// KSP_DIVERGED_DTOL / NANORINF like any KSP (dtol 1e5) instead of returning garbage after maxit steps.
// One fused launch per step where the state came with v0 (k_mom3, OUT == 4: 144 B/cell), the product and a vector update otherwise.
// from_guess: x_dev holds x_0 (the recurrence starts from any x_0: rho_0 = 0, the first step is x_1 = x_0 + c M (b - A x_0)); the first norm is then
// the guess's residual norm, so the caller passes the tolerances it means in absolute terms (momentum_solve_from_guess)
static int momentum_cheb(fl_momentum *m, const double *b_dev, double *x_dev, const fl_ksp_opts *opts, fl_ksp_stats *stats, bool from_guess = false)
{
  if (opts->pc != FL_PC_JACOBI && opts->pc != FL_PC_NONE) return FL_ERR_SUP;
  if (opts->norm_type == FL_NORM_NATURAL) return FL_ERR_SUP;
  if (opts->maxit < 0) return FL_ERR_ARG_OUTOFRANGE;
  fl_poisson *h = m->p;
  FL_HIP(hipSetDevice(h->device));
  std::memset(stats, 0, sizeof(*stats));
  const bool jac = opts->pc == FL_PC_JACOBI;
  double     emin = opts->emin, emax = opts->emax;
  bool       default_interval = false;
  if (emin == 0. && emax == 0.) {
    if (!jac) return FL_ERR_SUP;  // no bound of the unscaled operator is formed: give -ksp_chebyshev_eigenvalues
    FL_CHK(fl_momentum_chebyshev_interval(m, &emin, &emax));
    default_interval = true;
  }
  if (!(emax > emin) || !(emin > 0.)) return FL_ERR_ARG_OUTOFRANGE;
  const bool fused = m->fly && mom3_grid(h->g);
  for (int a : {0, 2, 4}) FL_CHK(mom_vec(m, a));
  if (!fused) FL_CHK(mom_vec(m, 3));
  double *B = m->vec[0], *X0 = m->vec[4], *X1 = m->vec[2], *AX = m->vec[3];
  const int nhist = opts->maxit + 2;
  FL_CHK(fl_ensure_hist(h, nhist));
  FL_CHK(fl_ensure_partials(h, m->t2blocks));
  fl_ksp_opts o = *opts;
  o.remove_nullspace = 0;  // A = I + ... is non-singular
  const bool watched = default_interval && o.norm_type == FL_NORM_NONE;
  if (watched) {  // the heuristic interval with no norm asked for: watch the preconditioned norm anyway, stop on divergence only
    o.norm_type = FL_NORM_PRECONDITIONED;
    o.rtol      = 0.;
    o.atol      = 0.;
  }
  FL_CHK(fl_cheb_begin(h, &o, emin, emax));
  const size_t bytes = sizeof(double) * 3 * h->padlen;
  // x_0 = 0 (or the caller's guess) and "x_-1" (multiplied by rho_0 = 0) must be finite numbers
  for (double *v : {X0, X1}) FL_HIP(hipMemsetAsync(v, 0, bytes, h->stream));
  for (int c = 0; c < 3; ++c) launch_pad_copy(h->stream, h->g, b_dev + (size_t)c * h->ncell, B + (size_t)c * h->padlen);
  if (from_guess)
    for (int c = 0; c < 3; ++c) launch_pad_copy(h->stream, h->g, x_dev + (size_t)c * h->ncell, X0 + (size_t)c * h->padlen);
  const int every = o.check_every > 0 ? o.check_every : 8;
  const int total = o.norm_type == FL_NORM_NONE ? o.maxit : o.maxit + 1;  // with a norm, launch maxit is only the final test
  int       j = 0, hostcur = 0;
  bool      done = total <= 0;
  while (!done) {
    const int stop = std::min(total, j + every);
    for (; j < stop; ++j) {
      double *xin = hostcur ? X1 : X0, *xout = hostcur ? X0 : X1;
      if (j > 0 || from_guess) FL_CHK(mom_ghosts(m, xin));
      if (fused) mom_launch_cheb_step(m, jac, xin, xout, B);
      else {
        FL_CHK(mom_launch_apply(m, 0, false, 0, xin, AX, nullptr, h->scal));
        FL_CHK(mom_launch_pw(m, 6, xin, AX, B, jac ? m->dg.p : nullptr, xout, nullptr));
      }
      FL_CHK(fl_cheb_fin_step(h, m->t2blocks, nhist));
      hostcur ^= 1;
    }
    FL_HIP(hipGetLastError());
    FL_CHK(fl_poll_scal(h));
    if (h->scal_host->reason != 0 || j >= total) done = true;
  }
  FL_CHK(fl_poll_scal(h));
  const double *ans = h->scal_host->cur ? X1 : X0;
  for (int c = 0; c < 3; ++c) launch_unpad_copy(h->stream, h->g, ans + (size_t)c * h->padlen, x_dev + (size_t)c * h->ncell, nullptr);
  FL_CHK(fl_ksp_finish(h, &o, stats));
  if (watched && stats->reason == FL_DIVERGED_ITS) stats->reason = FL_CONVERGED_ITS;  // what KSP_NORM_NONE reports after maxit steps
  return 0;
}

// KSPGMRES as PETSc runs it by default: restart 30 (-ksp_gmres_restart), classical Gram-Schmidt without refinement, left
// preconditioning, the preconditioned residual norm from the Givens recurrence as the monitored norm, KSPConvergedDefault, the
// residual re-formed at every restart.  Host control flow over device vectors: per iteration one operator application, one
// VecMDot (one host wait), one VecMAXPY and one norm (a second wait) -- PETSc's own sequence.  The basis lives in unpadded
// component-major vectors; they are allocated as the iteration reaches them (PETSc's GMRES_DELTA_DIRECTIONS idea): a 512^3
// basis vector is 3.2 GB.
static int momentum_gmres(fl_momentum *m, const double *b_dev, double *x_dev, const fl_ksp_opts *opts, fl_ksp_stats *stats)
{
  if (opts->pc != FL_PC_JACOBI && opts->pc != FL_PC_NONE) return FL_ERR_SUP;
  if (opts->norm_type != FL_NORM_PRECONDITIONED) return FL_ERR_SUP;
  if (opts->maxit < 0) return FL_ERR_ARG_OUTOFRANGE;
  const int restart = opts->gmres_restart > 0 ? opts->gmres_restart : 30;
  if (restart > 1000) return FL_ERR_ARG_OUTOFRANGE;
  fl_poisson *h = m->p;
  FL_HIP(hipSetDevice(h->device));
  std::memset(stats, 0, sizeof(*stats));
  const bool    jac = opts->pc == FL_PC_JACOBI;
  const int64_t n = 3 * (int64_t)h->ncell;
  hipStream_t   s = h->stream;
  FL_CHK(mom_vec(m, 7));
  // kb[0] = w, kb[1] = x, kb[2] = r, kb[3] = M b, kb[4 + k] = v_k
  auto kvec = [&](size_t i) -> int {
    if (m->kb.size() <= i) m->kb.resize(i + 1);
    return m->kb[i].once(h, n, true);
  };
  for (size_t i = 0; i < 4; ++i) FL_CHK(kvec(i));
  double *W = m->kb[0], *X = m->kb[1], *R = m->kb[2];
  // y = M A x for unpadded x, y
  auto apply = [&](const double *xin, double *yout) -> int {
    FL_CHK(mom_stage(m, xin));
    return mom_launch_apply(m, 0, jac, 1, m->vec[7], yout, nullptr, nullptr);
  };
  // M b, once: b ./ diag(A) (PCJACOBI) or b
  double *MB = m->kb[3];
  if (jac) {
    FL_CHK(fl_momentum_diagonal(m, W));  // unpadded diag(A); W is free at this point
    hipLaunchKernelGGL(k_div, dim3(nblk_flat(n)), dim3(256), 0, s, n, b_dev, (const double *)W, MB);
  } else lincomb(h, n, 1., b_dev, 0., nullptr, MB);
  hipEvent_t e0 = h->ev0, e1 = h->ev1;
  FL_HIP(hipEventRecord(e0, s));
  GmresLsq                    lsq(restart);
  std::vector<double>         hist, hcol(restart + 1, 0.), y(restart, 0.);
  std::vector<const double *> basis(restart + 1, nullptr);
  FL_HIP(hipMemsetAsync(X, 0, sizeof(double) * (size_t)n, s));
  lincomb(h, n, 1., MB, 0., nullptr, R);  // x = 0: r = M b
  double beta = 0.;
  FL_CHK(fl_vec_dot(h, n, R, R, &beta));
  beta = std::sqrt(beta);
  const double rnorm0 = beta, ttol = std::max(opts->rtol * rnorm0, opts->atol);
  auto converged = [&](double v) {
    if (std::isnan(v) || std::isinf(v)) return (int)FL_DIVERGED_NANORINF;
    if (v <= ttol) return v < opts->atol ? (int)FL_CONVERGED_ATOL : (int)FL_CONVERGED_RTOL;
    if (v >= opts->dtol * rnorm0) return (int)FL_DIVERGED_DTOL;
    return 0;
  };
  hist.push_back(beta);
  int    it = 0, reason = converged(beta);
  double res = beta;
  if (!reason && opts->maxit == 0) reason = FL_DIVERGED_ITS;
  while (!reason) {
    // one restart cycle
    FL_CHK(kvec(4));
    lincomb(h, n, 1. / beta, R, 0., nullptr, m->kb[4]);
    lsq.reset(beta);
    int k = 0;
    for (; k < restart && !reason; ++k) {
      FL_CHK(kvec(4 + (size_t)k + 1));
      for (int i = 0; i <= k; ++i) basis[i] = m->kb[4 + (size_t)i];
      FL_CHK(apply(m->kb[4 + (size_t)k], W));
      FL_CHK(fl_vec_mdot(h, n, W, basis.data(), k + 1, hcol.data()));            // h_i = w . v_i   (classical Gram-Schmidt)
      for (int i = 0; i <= k; ++i) y[i] = -hcol[i];
      FL_CHK(fl_vec_maxpy(h, n, W, y.data(), basis.data(), k + 1));              // w -= sum h_i v_i
      double hk1 = 0.;
      FL_CHK(fl_vec_dot(h, n, W, W, &hk1));
      hk1 = std::sqrt(hk1);
      hcol[k + 1] = hk1;
      const bool happy = !(hk1 > 1e-30 * rnorm0);                                 // KSPGMRES happy breakdown: the Krylov space is invariant
      if (!happy) lincomb(h, n, 1. / hk1, W, 0., nullptr, m->kb[4 + (size_t)k + 1]);
      res = lsq.push(k, hcol.data());  // previous rotations, then the new one
      ++it;
      hist.push_back(res);
      reason = converged(res);
      if (!reason && happy) reason = FL_CONVERGED_RTOL;  // exact solution in the current space (PETSc: CONVERGED_HAPPY_BREAKDOWN maps to converged)
      if (!reason && it >= opts->maxit) reason = FL_DIVERGED_ITS;
    }
    // x += V y,  H y = g  (upper triangular, k columns)
    lsq.solve(k, y.data());
    for (int i = 0; i < k; ++i) basis[i] = m->kb[4 + (size_t)i];
    FL_CHK(fl_vec_maxpy(h, n, X, y.data(), basis.data(), k));
    if (reason) break;
    // restart: r = M (b - A x)
    FL_CHK(apply(X, W));                    // W = M A x
    lincomb(h, n, 1., MB, -1., W, R);
    FL_CHK(fl_vec_dot(h, n, R, R, &beta));
    beta = std::sqrt(beta);
    if (!(beta > 0.)) {
      reason = std::isnan(beta) ? FL_DIVERGED_NANORINF : FL_CONVERGED_ATOL;
      break;
    }
  }
  lincomb(h, n, 1., X, 0., nullptr, x_dev);
  FL_HIP(hipEventRecord(e1, s));
  FL_HIP(hipStreamSynchronize(s));
  FL_HIP(hipGetLastError());
  float ms = 0.f;
  FL_HIP(hipEventElapsedTime(&ms, e0, e1));
  stats->iters   = it;
  stats->reason  = reason;
  stats->rnorm0  = rnorm0;
  stats->rnorm   = res;
  stats->seconds = ms * 1e-3;
  if (opts->history && opts->nhistory > 0) std::memcpy(opts->history, hist.data(), sizeof(double) * std::min<size_t>((size_t)opts->nhistory, hist.size()));
  return FL_SUCCESS;
}

// -ksp_initial_guess_nonzero on kspA: x_dev holds x0.  The Krylov methods here start from zero, and a Krylov method started from x0 is the same method
// started from zero on the shifted system  A d = b - A x0,  x = x0 + d  (same residuals, same iterates).  What changes is the convergence test:
// KSPConvergedDefault compares with the norm of the right-hand side b in the KSP's norm when the guess is non-zero (not with the initial residual),
// so the shifted solve runs to the ABSOLUTE tolerance max(rtol ||M b||, atol).  Costs one product, a scaled norm of b and two vector updates in
// front of the solve; saves every iteration the guess is worth -- in a time step, where x0 = the previous velocity, b - A x0 = O(dt) b.
static int momentum_solve_from_guess(fl_momentum *m, const double *b_dev, double *x_dev, const fl_ksp_opts *opts, fl_ksp_stats *stats)
{
  fl_poisson *h = m->p;
  FL_HIP(hipSetDevice(h->device));
  const int64_t n3 = 3 * h->ncell;
  // || M b || (M = 1 / diag with PCJACOBI and a preconditioned norm, else the identity): the update kernel that starts BiCGStab forms b / diag and
  // its square sum in one pass (slot 1); its two outputs are scratch here
  const bool scaled = opts->pc == FL_PC_JACOBI && opts->norm_type != FL_NORM_UNPRECONDITIONED;
  for (int a = 0; a < 2; ++a) FL_CHK(mom_vec(m, a));
  FL_CHK(fl_ensure_partials(h, m->t2blocks));
  FL_CHK(mom_launch_pw(m, 3, b_dev, scaled ? m->dg.p : nullptr, nullptr, nullptr, m->vec[0], m->vec[1]));
  launch_reduce(h->stream, h->partial, m->t2blocks, h->partial_stride, 3, h->sums);
  if (h->multi) FL_CHK(h->comm.allreduce(h->stream, h->sums, NSLOT));
  double sums[NSLOT];
  FL_HIP(hipMemcpyAsync(sums, h->sums, sizeof(sums), hipMemcpyDeviceToHost, h->stream));
  FL_HIP(hipStreamSynchronize(h->stream));
  const double bnorm = std::sqrt(sums[1] > 0. ? sums[1] : 0.);
  if (opts->type == FL_KSP_CHEBYSHEV) {  // the recurrence takes the guess as it is: no shifted system, no product and no vector update in front of it
    fl_ksp_opts o = *opts;
    o.initial_guess_nonzero = 0;
    o.rtol = 0.;
    o.atol = std::max(opts->rtol * bnorm, opts->atol);
    FL_CHK(momentum_cheb(m, b_dev, x_dev, &o, stats, true));
    if (stats->reason == FL_CONVERGED_ATOL && !(stats->rnorm < opts->atol)) stats->reason = FL_CONVERGED_RTOL;
    stats->rnorm0 = bnorm;
    return FL_SUCCESS;
  }
  FL_CHK(m->gr.once(h, n3, false));
  FL_CHK(m->gd.once(h, n3, false));
  // r = b - A x0
  FL_CHK(fl_momentum_apply(m, x_dev, m->gr));
  lincomb(h, n3, 1., b_dev, -1., m->gr, m->gr);
  fl_ksp_opts o = *opts;
  o.initial_guess_nonzero = 0;
  o.rtol = 0.;
  o.atol = std::max(opts->rtol * bnorm, opts->atol);
  FL_CHK(fl_momentum_solve(m, m->gr, m->gd, &o, stats));
  lincomb(h, n3, 1., x_dev, 1., m->gd, x_dev);  // x = x0 + d
  FL_HIP(hipGetLastError());
  if (stats->reason == FL_CONVERGED_ATOL && !(stats->rnorm < opts->atol)) stats->reason = FL_CONVERGED_RTOL;  // it was the relative test that was met
  stats->rnorm0 = bnorm;  // what the relative tolerance refers to
  return FL_SUCCESS;
}

extern "C" int fl_momentum_solve(fl_momentum *m, const double *b_dev, double *x_dev, const fl_ksp_opts *opts, fl_ksp_stats *stats)
{
  if (!m || !b_dev || !x_dev || !opts || !stats) return FL_ERR_ARG_NULL;
  if (!m->have_state && m->mp.cC != 0.) return FL_ERR_ARG_WRONGSTATE;
  if (opts->initial_guess_nonzero) return momentum_solve_from_guess(m, b_dev, x_dev, opts, stats);
  if (opts->type == FL_KSP_GMRES) return momentum_gmres(m, b_dev, x_dev, opts, stats);
  if (opts->type == FL_KSP_CHEBYSHEV) return momentum_cheb(m, b_dev, x_dev, opts, stats);
  if (opts->type != FL_KSP_BCGS) return FL_ERR_SUP;
  if (opts->pc != FL_PC_JACOBI && opts->pc != FL_PC_NONE) return FL_ERR_SUP;
  if (opts->norm_type != FL_NORM_PRECONDITIONED) return FL_ERR_SUP;
  if (opts->maxit < 0) return FL_ERR_ARG_OUTOFRANGE;
  fl_poisson *h = m->p;
  FL_HIP(hipSetDevice(h->device));
  std::memset(stats, 0, sizeof(*stats));
  const bool jac = opts->pc == FL_PC_JACOBI;
  for (int a = 0; a < 7; ++a) FL_CHK(mom_vec(m, a));
  double *R = m->vec[0], *RP = m->vec[1], *P = m->vec[2], *V = m->vec[3], *X = m->vec[4], *S = m->vec[5], *T = m->vec[6];
  const int nhist = opts->maxit + 1;
  FL_CHK(fl_ensure_hist(h, nhist));
  FL_CHK(fl_ensure_partials(h, m->t2blocks));
  fl_ksp_opts o = *opts;
  o.remove_nullspace = 0;  // A = I + ... is non-singular
  FL_CHK(fl_ksp_begin(h, &o));
  // P, V and X start as zero vectors: the first iteration says so in its kernels (P = R; X is written, not read) and nothing is zeroed -- three
  // 3N memsets and the reads of them less per solve
  const size_t bytes = sizeof(double) * 3 * h->padlen;
  FL_CHK(mom_launch_pw(m, 3, b_dev, jac ? m->dg.p : nullptr, nullptr, nullptr, R, RP));
  FL_CHK(fl_bcgs_fin_step(h, 0, m->t2blocks, 3, nhist));
  const int every = o.check_every > 0 ? o.check_every : 4;
  int       it = 0;
  bool      done = false;
  while (!done) {
    const int stop = std::min(o.maxit, it + every);
    for (; it < stop; ++it) {
      if (it == 0) FL_CHK(mom_launch_pw(m, 4, R, nullptr, nullptr, nullptr, P, nullptr));
      else FL_CHK(mom_launch_pw(m, 0, R, V, nullptr, nullptr, P, nullptr));
      FL_CHK(mom_ghosts(m, P));
      FL_CHK(mom_launch_apply(m, 1, jac, 0, P, V, RP, h->scal));
      FL_CHK(fl_bcgs_fin_step(h, 1, m->t2blocks, 4, nhist));
      FL_CHK(mom_launch_pw(m, 1, R, V, nullptr, nullptr, S, nullptr));
      FL_CHK(mom_ghosts(m, S));
      FL_CHK(mom_launch_apply(m, 2, jac, 0, S, T, nullptr, h->scal));
      FL_CHK(fl_bcgs_fin_step(h, 3, m->t2blocks, 4, nhist));
      FL_CHK(mom_launch_pw(m, it == 0 ? 5 : 2, P, S, T, RP, X, R));
      FL_CHK(fl_bcgs_fin_step(h, 4, m->t2blocks, 3, nhist));
    }
    FL_CHK(fl_poll_scal(h));
    if (h->scal_host->reason != 0 || it >= o.maxit) done = true;
  }
  if (h->scal_host->it == 0) FL_HIP(hipMemsetAsync(X, 0, bytes, h->stream));  // stopped before the first update wrote X: the answer is the zero guess
  for (int c = 0; c < 3; ++c) launch_unpad_copy(h->stream, h->g, X + (size_t)c * h->padlen, x_dev + (size_t)c * h->ncell, nullptr);
  return fl_ksp_finish(h, &o, stats);
}
