// fl_gmres_lsq.h -- the small least-squares problem of a GMRES cycle, min_y || beta e_1 - H y ||, H the (k+1) x k upper-Hessenberg matrix of the Arnoldi
// relation: a QR factorisation by Givens rotations, one column at a time.  Shared by the two host-driven GMRES loops (momentum_gmres in
// fl_mom_solve.hip, schur_solve_var in fl_abf.hip); plain C++ without HIP, so that tests/plugins/gmres_lsq_check.cpp exercises it with the host
// compiler alone.  The orthogonalisation, the convergence tests and the breakdown rules stay with the drivers.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <vector>

#pragma GCC visibility push(hidden)  // internal to the library: its dynamic symbols stay the C-ABI's

namespace fl {

struct GmresLsq {
  int                 m;          // columns at most (the restart length)
  std::vector<double> cs, sn, g;  // the rotations; Q^T beta e_1
  std::vector<double> R;          // the triangular factor, row-major m x m

  explicit GmresLsq(int restart) : m(restart), cs((size_t)restart, 0.), sn((size_t)restart, 0.), g((size_t)restart + 1, 0.), R((size_t)restart * restart, 0.) {}

  // a new cycle from a residual of norm beta
  void reset(double beta)
  {
    std::fill(g.begin(), g.end(), 0.);
    g[0] = beta;
  }

  // Column k of H in h[0 .. k+1] (overwritten with the rotated column): the earlier rotations, then the one that annihilates h[k+1].  Returns the norm
  // of the least-squares residual with k + 1 columns, |g[k+1]|.
  double push(int k, double *h)
  {
    for (int i = 0; i < k; ++i) {
      const double a = h[i], c = h[i + 1];
      h[i]     = cs[i] * a + sn[i] * c;
      h[i + 1] = -sn[i] * a + cs[i] * c;
    }
    const double a = h[k], c = h[k + 1], d = std::hypot(a, c);
    cs[k]    = d > 0. ? a / d : 1.;
    sn[k]    = d > 0. ? c / d : 0.;
    h[k]     = d;
    h[k + 1] = 0.;
    g[k + 1] = -sn[k] * g[k];
    g[k]     = cs[k] * g[k];
    for (int i = 0; i <= k; ++i) R[(size_t)i * m + k] = h[i];
    return std::fabs(g[k + 1]);
  }

  // y[0 .. k): R y = g over the first k columns, from the last row up
  void solve(int k, double *y) const
  {
    for (int i = k - 1; i >= 0; --i) {
      double t = g[i];
      for (int j = i + 1; j < k; ++j) t -= R[(size_t)i * m + j] * y[j];
      y[i] = t / R[(size_t)i * m + i];
    }
  }
};

}  // namespace fl

#pragma GCC visibility pop
