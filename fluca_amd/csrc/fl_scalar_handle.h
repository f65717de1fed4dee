// fl_scalar_handle.h -- the fl_scalar handle and what the kernels of fl_scalar.hip and fl_scalar_implicit.hip share: the grid as a kernel sees it and
// the read of a cell of the caller's unpadded array.
#pragma once
#include "fl_devbuf.h"
#include "fl_handle.h"
#include "fl_limiter.h"

namespace fl {

struct ScGrid {
  int           nx, ny, nz, per;  // per: bit d = axis d is periodic
  int           kind[6];          // per boundary: 0 Dirichlet, 1 Neumann (derivative along +axis), 2 periodic
  double        val[6];
  double        dlo[3], dhi[3];   // distance first centre -- low boundary face, high boundary face -- last centre
  double        gamma;
  const ScCell *c[3];
};

// w at cell m of a line of n cells (c0: index of its cell 0, cs: stride): outside the line the periodic image, or -- at a boundary -- the
// nearest cell (a placeholder that keeps the address legal; sc_axis replaces what the boundary rule defines and never uses the rest)
__device__ __forceinline__ double sc_ld(const double *__restrict__ w, int64_t c0, int64_t cs, int m, int n, bool wraps)
{
  if (m < 0) {
    m = wraps ? m + n : 0;
    if (m < 0) m += n;  // (n == 1)
  } else if (m >= n) {
    m = wraps ? m - n : n - 1;
    if (m >= n) m -= n;
  }
  return w[c0 + m * cs];
}

// Several ranks: what differs from the one-rank sweep is where the cells outside the block come from.  One end of an axis of a rank's block:
// nlo / nhi a neighbouring rank sits behind the low / high end, r the four layers received across them (np: lines of the plane, pr: this lane's line)
struct ScEnds {
  bool          nlo, nhi;
  const double *r;
  int64_t       np, pr;
};
// w at cell m of the line: behind an end with a neighbouring rank the cell -2, -1 / n, n+1 is layer m + 2 / m - n + 2 of e.r; elsewhere as
// sc_ld.  Branches, not a selected address: along y and z they are wave-uniform, along x only the waves at the ends of a row take them.
__device__ __forceinline__ double sc_ld_ring(const double *__restrict__ w, int64_t c0, int64_t cs, int m, int n, bool wraps, const ScEnds &e)
{
  if (m < 0 && e.nlo) return e.r[(m + 2) * e.np + e.pr];
  if (m >= n && e.nhi) return e.r[(m - n + 2) * e.np + e.pr];
  return sc_ld(w, c0, cs, m, n, wraps);
}

}  // namespace fl

#pragma GCC visibility push(hidden)  // the handle is internal to the library (what its kernels take, above, is not)

struct fl_scalar {
  fl_poisson   *h = nullptr;  // borrowed: grid, device, stream
  fl::ScGrid    g;
  int           limiter = fl::LIM_SUPERBEE;
  const double *V[3] = {nullptr, nullptr, nullptr};  // borrowed
  // device arrays the handle owns (DevBuf: freed with the handle)
  fl::DevBuf<fl::ScCell> tab[3];
  fl::DevBuf<double>     hw[3];    // face-to-face widths
  fl::DevBuf<double>     work[2];  // the two stage vectors of fl_scalar_step
  fl::DevBuf<double>     partial;  // 3 * SC_REDUCE_BLOCKS
  std::vector<double> partial_host;
  const double *hwl[3] = {nullptr, nullptr, nullptr};  // hw cut to the rank's cells
  // one rank's block of several (fl_scalar_create_ranks): nb as k_scalar_stage_ring takes it; the layers received and sent (ScRing)
  bool    ring = false;
  int     nb = 0;
  fl::DevBuf<double> slab_recv, slab_send;
  // the implicit path (fl_scalar_implicit.hip), made on first use: the right-hand side of fl_scalar_step_imex (its second array beside work[]: the
  // Chebyshev direction and the other iterate live in work[0], work[1], which the explicit stages have left by then); max_i omega_d(i) per axis
  fl::DevBuf<double> imex_b;
  bool    have_omega = false;
  double  omega[3] = {0., 0., 0.};
};

#pragma GCC visibility pop

namespace fl {

// fl_scalar.hip: the stages of fl_scalar_step over dt, reading phi^n from phi_dev and writing the new phi to out_dev (phi_dev itself, or an array that
// is neither phi_dev nor a work array); the arguments are checked by the callers.  pack_last (several ranks): the last stage fills the send slabs
// with what it writes, as every other stage does -- for a caller that exchanges out_dev next (fl_scalar_step_imex_ranks)
int scalar_ssp_step(fl_scalar *m, double dt, int nstages, const double *source_dev, const double *phi_dev, double *out_dev, bool pack_last);

// fl_scalar.hip, several ranks, ONE layer per rank face (the 7-point star of fl_scalar_implicit.hip): the cell 0 / n - 1 of an axis is the send layer
// 0 / 3 of that axis, the cell -1 / n the receive layer 1 / 2 -- where the two-layer exchange of the stages keeps the same cells, so a stage that
// packs leaves what scalar_ring_exchange1 sends.  scalar_ring_pack1: those send layers from the caller's array (a launch, no message);
// scalar_ring_exchange1: one message of one plane per rank face, on the handle's stream.
int scalar_ring_pack1(fl_scalar *m, const double *phi_dev);
int scalar_ring_exchange1(fl_scalar *m);

}  // namespace fl
