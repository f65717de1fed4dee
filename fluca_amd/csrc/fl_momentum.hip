// fl_momentum.hip -- the momentum block of the Jacobian, matrix-free:  A = I + dt C - (mu dt / 2 rho) L
//
//   NSFormJacobian_CNLinear_Cart3d_Internal    cnlinearcart3d.c:2930-2941
//   ComputeVelocityLaplacianOperator_Private   cnlinearcart3d.c:425-632      L: one 1-D second-derivative row per axis
//   ComputeConvectionOperator_Private          cnlinearcart3d.c:873-1294     (C v)_c = 1/2 d/dx_d (v_c V0_d + v0interp_c v_d)
//
// The reference assembles A as an AIJ matrix every time step (MatZeroEntries + 24 MatSetValuesStencil per row).  Here
// nothing is assembled: the rows are products of 1-D tables (fl_coeff.cpp: build_axis_momentum) with the face fields V0
// and v0interp, evaluated on the fly.  Velocity vectors are three padded cell arrays (component-major), the twelve face
// fields are kept as padded arrays whose entry (i,j,k) is the LOW face of cell (i,j,k) along the field's axis, so the high
// face is the next entry along that axis (ghost layer = the last face / the periodic image / the neighbour rank's first
// face).  Algorithmic HBM traffic of one application: 3 reads + 3 writes of v, 12 face reads = 144 B per cell.
//
// This unit is the operator and nothing else: its kernels, the handle, the state, the product and what is read off the rows (diagonal, row sums,
// Gershgorin radius, the right-hand side).  The Krylov drivers on it are fl_mom_solve.hip, the block preconditioner around it fl_abf.hip; they
// reach the kernels here through the launchers of fl_mom_handle.h, so an edit to a solver leaves the text the counter passes of k_mom2 / k_mom3
// are tied to (fluca_amd/provenance.py) as it is.
#include <new>

#include "fl_mom_handle.h"
#include "fl_device.h"

namespace fl {

// 1/d: hardware estimate + two Newton steps (correctly rounded for all but a vanishing fraction of inputs)
__device__ __forceinline__ double recip(double d)
{
  double r = __builtin_amdgcn_rcp(d);
  r        = fma(r, fma(-d, r, 1.), r);
  r        = fma(r, fma(-d, r, 1.), r);
  return r;
}

}  // namespace fl
#include "fl_stencil.h"
#include "fl_mom_tile.h"
#include "fl_mom_tile3.h"
namespace fl {

// BiCGStab vector updates on three-component padded vectors (interior cells only).
// OP 0: P = R - (omega_old beta) V + beta P
// OP 1: S = R - alpha V
// OP 2: X += alpha P + omega S ; R = S - omega T          slots: 0 R.R  1 R.RP  2 sum R
// OP 3: R = RP = b / diag (b unpadded, component-major)    slots: 0 sum R  1 R.R        (dg NULL: no preconditioner)
//
// The tile walk of k_mom2: a block marches a 128 x 8 tile through a z chunk, two x-adjacent cells per lane (16-byte accesses, non-temporal
// where a value is not read again before it would be evicted anyway), blocks in the XCD-contiguous order -- the access pattern at which the
// stencil kernels move 6 TB/s where a grid-stride walk over row segments moved 5.3.  Padded rows start on a 128-byte boundary (PADX), so every
// pair is 16-byte aligned; the unpadded b of OP 3 is read in pairs when nx is even (pairs != 0).
template <int OP>
__global__ void __launch_bounds__(512) k_mom_pw3(GridP g, int64_t cs, const double *__restrict__ a0, const double *__restrict__ a1, const double *__restrict__ a2, const double *__restrict__ a3, double *__restrict__ w0,
                                                 double *__restrict__ w1, const KspScal *__restrict__ s, double *__restrict__ partial, int pstride, int pairs, int tiles_x, int nchunk, int zc)
{
  __shared__ double red[3 * 8];
  if (OP != 3 && s->reason != 0) return;
  const double alpha = s->alpha, omega = s->omega, beta = s->beta, ob = s->omega_old * s->beta;
  const int    nb = gridDim.x, tiles = nb / nchunk, b = xcd_remap(blockIdx.x, nb), chunk = b / tiles, tile = b % tiles;
  const int    lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int    i = (tile % tiles_x) * 128 + 2 * lane, j = (tile / tiles_x) * 8 + w;
  const int    k0 = chunk * zc, k1 = min(k0 + zc, g.nz);
  const int64_t ncell = (int64_t)g.nx * g.ny * g.nz;
  double       acc[3] = {0., 0., 0.};
  if (i < g.nx && j < g.ny) {
    const bool two = i + 1 < g.nx;
    auto       ldp = [&](const double *p, int64_t q) { return two ? ld2<1>(p + q) : make_double2(p[q], 0.); };
    auto       ldk = [&](const double *p, int64_t q) { return two ? ld2<0>(p + q) : make_double2(p[q], 0.); };
    auto       stp = [&](double *p, int64_t q, double2 v) {
      if (two) st2<0>(p + q, v);
      else p[q] = v.x;
    };
    for (int k = k0; k < k1; ++k) {
      const int64_t idx = g.off0 + (int64_t)k * g.sxy + (int64_t)j * g.sx + i, ub = ((int64_t)k * g.ny + j) * g.nx + i;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const int64_t q = c * cs + idx;
        if (OP == 0) {
          const double2 r = ldk(a0, q), v = ldp(a1, q), p = ldp(w0, q);
          stp(w0, q, make_double2(r.x - ob * v.x + beta * p.x, r.y - ob * v.y + beta * p.y));
        } else if (OP == 4) {  // the first iteration's OP 0: P and V are zero by definition, so P = R (nothing is zeroed or read for it)
          stp(w0, q, ldk(a0, q));
        } else if (OP == 1) {
          const double2 r = ldp(a0, q), v = ldp(a1, q);
          stp(w0, q, make_double2(r.x - alpha * v.x, r.y - alpha * v.y));
        } else if (OP == 6) {  // one Chebyshev step behind an un-fused product (see k_mom3, OUT == 4): a0 = x_k, a1 = A x_k, a2 = b, a3 = diag(A) or NULL, w0 = x_{k-1} -> x_{k+1}
          const double2 xk = ldp(a0, q), ax = ldp(a1, q), bb = ldp(a2, q), xo = ldp(w0, q);
          const double2 rr = make_double2(bb.x - ax.x, bb.y - ax.y);
          double2       zz = rr;
          if (a3) {
            const double2 d = ldk(a3, q);
            zz.x = rr.x * recip(d.x);
            zz.y = two ? rr.y * recip(d.y) : 0.;
          }
          stp(w0, q, make_double2(fma(s->cheb_c, zz.x, fma(s->cheb_rho, xk.x - xo.x, xk.x)), fma(s->cheb_c, zz.y, fma(s->cheb_rho, xk.y - xo.y, xk.y))));
          acc[0] += zz.x + (two ? zz.y : 0.);
          acc[1] += zz.x * zz.x + (two ? zz.y * zz.y : 0.);
          acc[2] += rr.x * rr.x + (two ? rr.y * rr.y : 0.);
        } else if (OP == 2 || OP == 5) {  // OP 5: the first iteration's OP 2 -- X is zero by definition and not read
          const double2 P = ldp(a0, q), S = ldp(a1, q), T = ldp(a2, q), RP = ldk(a3, q), X = OP == 5 ? make_double2(0., 0.) : ldp(w0, q);
          const double2 rn = make_double2(S.x - omega * T.x, S.y - omega * T.y);
          double2       xn = X;
          xn.x += alpha * P.x + omega * S.x;
          xn.y += alpha * P.y + omega * S.y;
          if (two) st2<1>(w0 + q, xn);
          else w0[q] = xn.x;
          stp(w1, q, rn);
          acc[0] += rn.x * rn.x + (two ? rn.y * rn.y : 0.);
          acc[1] += rn.x * RP.x + (two ? rn.y * RP.y : 0.);
          acc[2] += rn.x + (two ? rn.y : 0.);
        } else {
          const int64_t u = c * ncell + ub;
          double2       bb;
          if (two && pairs) bb = ld2<1>(a0 + u);
          else bb = make_double2(a0[u], two ? a0[u + 1] : 0.);
          double2 r = bb;
          if (a1) {
            const double2 d = ldp(a1, q);
            r.x = bb.x / d.x;
            if (two) r.y = bb.y / d.y;
          }
          stp(w0, q, r);
          stp(w1, q, r);
          acc[0] += r.x + (two ? r.y : 0.);
          acc[1] += r.x * r.x + (two ? r.y * r.y : 0.);
        }
      }
    }
  }
  if (OP == 2 || OP == 3 || OP == 5 || OP == 6) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const double v = wave_sum(acc[a]);
      if (lane == 0) red[a * 8 + w] = v;
    }
    __syncthreads();
    if (threadIdx.x < 3) {
      double v = 0.;
#pragma unroll
      for (int q = 0; q < 8; ++q) v += red[threadIdx.x * 8 + q];
      partial[(int64_t)threadIdx.x * pstride + blockIdx.x] = v;
    }
  }
}

// out = v
__global__ void __launch_bounds__(256) k_fill(int64_t n, double v, double *__restrict__ out)
{
  for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < n; q += (int64_t)gridDim.x * blockDim.x) out[q] = v;
}
// max of a and sum of b over the owned cells of three padded components each (partial[2 * block], partial[2 * block + 1]; either array may be NULL):
// four rows per pass, 16-byte loads -- eight loads in flight per thread (round 4; one row and 8-byte loads per pass ran at 3.2 TB/s)
__global__ void __launch_bounds__(256) k_max_sum_owned(GridP g, int64_t cs, const double *__restrict__ a, const double *__restrict__ b, double *__restrict__ partial)
{
  __shared__ double red[2][4];
  const int64_t plane = (int64_t)g.nz * g.ny, rows = 3 * plane;
  double        mx = 0., sm = 0.;
  for (int64_t r0 = (int64_t)blockIdx.x * 4; r0 < rows; r0 += (int64_t)gridDim.x * 4) {
    int64_t base[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t r = min(r0 + u, rows - 1);  // a repeated row changes neither the maximum nor (skipped below) the sum
      const int     c = (int)(r / plane), kj = (int)(r % plane), k = kj / g.ny, j = kj % g.ny;
      base[u] = (int64_t)c * cs + g.off0 + (int64_t)k * g.sxy + (int64_t)j * g.sx;
    }
    for (int i = 2 * threadIdx.x; i < g.nx; i += 512) {
      const bool two = i + 1 < g.nx;
      double2    va[4], vb[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        va[u] = a ? (two ? *reinterpret_cast<const double2 *>(a + base[u] + i) : make_double2(a[base[u] + i], 0.)) : make_double2(0., 0.);
        vb[u] = b ? (two ? *reinterpret_cast<const double2 *>(b + base[u] + i) : make_double2(b[base[u] + i], 0.)) : make_double2(0., 0.);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        mx = fmax(mx, fmax(va[u].x, va[u].y));
        if (r0 + u < rows) sm += vb[u].x + vb[u].y;
      }
    }
  }
  for (int off = 32; off > 0; off >>= 1) {
    mx = fmax(mx, __shfl_down(mx, off, 64));
    sm += __shfl_down(sm, off, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    red[0][threadIdx.x >> 6] = mx;
    red[1][threadIdx.x >> 6] = sm;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    partial[2 * blockIdx.x]     = fmax(fmax(red[0][0], red[0][1]), fmax(red[0][2], red[0][3]));
    partial[2 * blockIdx.x + 1] = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
  }
}

// src: x-fastest array of ex*ey*ez entries (ex <= nx+1, ...) -> padded array, entry (i,j,k) at off0 + k sxy + j sx + i
__global__ void __launch_bounds__(256) k_pad_copy_ext(GridP g, const double *__restrict__ src, double *__restrict__ dst, int ex, int ey, int ez)
{
  const int64_t n = (int64_t)ex * ey * ez;
  for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < n; q += (int64_t)gridDim.x * blockDim.x) {
    const int     i = (int)(q % ex);
    const int64_t r = q / ex;
    const int     j = (int)(r % ey), k = (int)(r / ey);
    dst[g.off0 + (int64_t)k * g.sxy + (int64_t)j * g.sx + i] = src[q];
  }
}

// The same for the faces at the two ends of axis d only (index 0 and, where the array holds it, index n_d): what k_mom3 reads of a stored
// v0interp field.  One thread per face of the two planes.
__global__ void __launch_bounds__(256) k_pad_copy_ends(GridP g, const double *__restrict__ src, double *__restrict__ dst, int ex, int ey, int ez, int d)
{
  const int     nd = d == 0 ? g.nx : (d == 1 ? g.ny : g.nz), ed = d == 0 ? ex : (d == 1 ? ey : ez);
  const int     na = d == 0 ? ey : ex, nb = d == 2 ? ey : ez;  // the two transverse extents, a fastest
  const int     nend = ed > nd ? 2 : 1;
  const int64_t n = (int64_t)na * nb * nend;
  for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < n; q += (int64_t)gridDim.x * blockDim.x) {
    const int a = (int)(q % na), b = (int)((q / na) % nb), f = (q / ((int64_t)na * nb)) ? nd : 0;
    const int i = d == 0 ? f : a, j = d == 1 ? f : (d == 0 ? a : b), k = d == 2 ? f : b;
    dst[g.off0 + (int64_t)k * g.sxy + (int64_t)j * g.sx + i] = src[((int64_t)k * ey + j) * ex + i];
  }
}

}  // namespace fl

using namespace fl;

// ------------------------------------------------------------------------------------------------ launches

int fl::mom_vec(fl_momentum *m, int slot) { return m->vec[slot].once(m->p, 3 * (int64_t)m->p->padlen, true); }

int fl::mom_ghosts(fl_momentum *m, double *v3)
{
  fl_poisson *h = m->p;
  if (!fl_any_ghost_exchange(h)) return 0;
  if (!h->multi) {  // periodic images inside the one block: the three components in one launch per axis
    for (int d = 0; d < 3; ++d)
      if (h->wrap_local[d]) launch_wrap(h->stream, h->g, v3, d, 3, (int64_t)h->padlen);
    return 0;
  }
  for (int c = 0; c < 3; ++c) FL_CHK(fl_fill_ghosts(h, v3 + (size_t)c * h->padlen));
  return 0;
}

int fl::mom_stage(fl_momentum *m, const double *v_dev)
{
  fl_poisson *h = m->p;
  FL_CHK(mom_vec(m, 7));
  for (int c = 0; c < 3; ++c) launch_pad_copy(h->stream, h->g, v_dev + (size_t)c * h->ncell, m->vec[7] + (size_t)c * h->padlen);
  return mom_ghosts(m, m->vec[7]);
}

namespace {

// block order of the tile walks (flags bit 0): chunk-major, XCD-contiguous; three alternating rounds at 512^3 against chunk-fastest: apply 5.83
// against 6.03 ms (profiles/r02c_mom_order.txt)
constexpr int MOM_XCD_ORDER = 1;

// DOT: 0 no inner products, 1 sum y and y.o (slots 0, 1), 2 x.y and y.y (slots 2, 3), 3 all four
template <int DOT, bool JAC, int OUT>
void mom_apply_t(fl_momentum *m, const double *x, double *y, const double *o, const KspScal *s, const MomP *coeffs = nullptr)
{
  fl_poisson *h = m->p;
  int         flags = MOM_XCD_ORDER;
  if (OUT == 1 && (h->g.nx & 1) == 0 && (reinterpret_cast<uintptr_t>(y) & 15) == 0) flags |= 2;
  if (m->fly && mom3_grid(h->g))
    hipLaunchKernelGGL((k_mom3<8, DOT, JAC, OUT, 1>), dim3(m->t2blocks), dim3(512), 0, h->stream, h->g, coeffs ? *coeffs : m->mp, x, y, (const double *)m->F, (const double *)m->v0p, (int64_t)h->padlen, o, s, h->partial,
                       h->partial_stride, m->t2x, m->t2chunk, m->t2zc, flags);
  else
    hipLaunchKernelGGL((k_mom2<8, DOT, JAC, OUT, 1>), dim3(m->t2blocks), dim3(512), 0, h->stream, h->g, coeffs ? *coeffs : m->mp, x, y, (const double *)m->F, (int64_t)h->padlen, o, s, h->partial, h->partial_stride, m->t2x,
                       m->t2chunk, m->t2zc, flags);
}

// the scaled, cell-major tables of k_mom2 for the coefficients in p (stream-ordered; slot 0: the handle's own, slot 1: a one-off operator)
int mom_scale_tables(fl_momentum *m, int slot, MomP &p)
{
  fl_poisson *h = m->p;
  for (int d = 0; d < 3; ++d) {
    const int len = m->mp.len[d], n = len * MOM_STAB;
    hipLaunchKernelGGL(k_mom_scale_tab, dim3((n + 255) / 256), dim3(256), 0, h->stream, (const double *)m->tabs[d], len, p.cC, p.cL, m->stabs[slot][d].p);
    p.stab[d] = m->stabs[slot][d];
  }
  FL_HIP(hipGetLastError());
  return 0;
}

template <int OP>
void mom_pw(fl_momentum *m, const double *a0, const double *a1, const double *a2, const double *a3, double *w0, double *w1)
{
  fl_poisson *h = m->p;
  const int   pairs = (h->g.nx & 1) == 0 && (reinterpret_cast<uintptr_t>(a0) & 15) == 0;
  hipLaunchKernelGGL((k_mom_pw3<OP>), dim3(m->t2blocks), dim3(512), 0, h->stream, h->g, (int64_t)h->padlen, a0, a1, a2, a3, w0, w1, h->scal, h->partial, h->partial_stride, pairs, m->t2x, m->t2chunk, m->t2zc);
}

}  // namespace

// The template arguments as run-time values: exactly the combinations the library is built with (a product with DOT == 3, or one that scales the
// diagonal by itself, has no caller and no kernel)
int fl::mom_launch_apply(fl_momentum *m, int dot, bool jac, int out, const double *x, double *y, const double *o, const KspScal *s)
{
  switch (dot * 100 + (jac ? 10 : 0) + out) {
    case 0: mom_apply_t<0, false, 0>(m, x, y, o, s); return 0;
    case 1: mom_apply_t<0, false, 1>(m, x, y, o, s); return 0;
    case 2: mom_apply_t<0, false, 2>(m, x, y, o, s); return 0;
    case 3: mom_apply_t<0, false, 3>(m, x, y, o, s); return 0;
    case 10: mom_apply_t<0, true, 0>(m, x, y, o, s); return 0;
    case 11: mom_apply_t<0, true, 1>(m, x, y, o, s); return 0;
    case 100: mom_apply_t<1, false, 0>(m, x, y, o, s); return 0;
    case 110: mom_apply_t<1, true, 0>(m, x, y, o, s); return 0;
    case 200: mom_apply_t<2, false, 0>(m, x, y, o, s); return 0;
    case 210: mom_apply_t<2, true, 0>(m, x, y, o, s); return 0;
  }
  return FL_ERR_SUP;
}

void fl::mom_launch_cheb_step(fl_momentum *m, bool jac, const double *xin, double *xout, const double *b)
{
  fl_poisson *h = m->p;
  if (jac) hipLaunchKernelGGL((k_mom3<8, 0, true, 4, 1>), dim3(m->t2blocks), dim3(512), 0, h->stream, h->g, m->mp, xin, xout, (const double *)m->F, (const double *)m->v0p, (int64_t)h->padlen, b, (const KspScal *)h->scal,
                              h->partial, h->partial_stride, m->t2x, m->t2chunk, m->t2zc, MOM_XCD_ORDER);
  else hipLaunchKernelGGL((k_mom3<8, 0, false, 4, 1>), dim3(m->t2blocks), dim3(512), 0, h->stream, h->g, m->mp, xin, xout, (const double *)m->F, (const double *)m->v0p, (int64_t)h->padlen, b, (const KspScal *)h->scal,
                          h->partial, h->partial_stride, m->t2x, m->t2chunk, m->t2zc, MOM_XCD_ORDER);
}

int fl::mom_launch_pw(fl_momentum *m, int op, const double *a0, const double *a1, const double *a2, const double *a3, double *w0, double *w1)
{
  switch (op) {
    case 0: mom_pw<0>(m, a0, a1, a2, a3, w0, w1); return 0;
    case 1: mom_pw<1>(m, a0, a1, a2, a3, w0, w1); return 0;
    case 2: mom_pw<2>(m, a0, a1, a2, a3, w0, w1); return 0;
    case 3: mom_pw<3>(m, a0, a1, a2, a3, w0, w1); return 0;
    case 4: mom_pw<4>(m, a0, a1, a2, a3, w0, w1); return 0;
    case 5: mom_pw<5>(m, a0, a1, a2, a3, w0, w1); return 0;
    case 6: mom_pw<6>(m, a0, a1, a2, a3, w0, w1); return 0;
  }
  return FL_ERR_SUP;
}

// k_mom2 / k_mom3 / k_mom_pw3: 128 x 8 tiles; about four blocks per CU in all (one is resident at a time: 158 KB of LDS) -- 512^3: 3.35 ms with
// 4 z chunks, 3.59 with 2, 3.50 with 8 (profiles/r03_mom_plan.txt); fewer, taller chunks where the partial-sum buffers (MAX_PARTIAL_BLOCKS
// entries per slot) would not hold a block each
MomPlan fl::mom_plan(const GridP &g)
{
  MomPlan p;
  p.t2x           = (g.nx + 127) / 128;
  const int tiles = p.t2x * ((g.ny + 7) / 8);
  int       nc    = z_chunk_count(tiles, g.nz, 1024);
  if (tiles * nc > MAX_PARTIAL_BLOCKS) nc = std::max(1, MAX_PARTIAL_BLOCKS / tiles);
  const ZChunks z = z_chunks(g.nz, nc);
  p.t2zc     = z.zc;
  p.t2chunk  = z.nchunk;
  p.t2blocks = tiles * p.t2chunk;
  return p;
}

// ------------------------------------------------------------------------------------------------ handle

namespace {

// a table of the handle: n elements (at least `least`) by hipMalloc, filled by a blocking copy
template <class T>
int mom_upload(fl_poisson *h, DevBuf<T> &dev, const std::vector<T> &host, size_t least)
{
  FL_CHK(dev.plain(h, (int64_t)std::max(host.size(), least)));
  FL_HIP(hipMemcpy(dev.p, host.data(), sizeof(T) * host.size(), hipMemcpyHostToDevice));
  return 0;
}

int mom_init(fl_momentum *m, fl_poisson *h)
{
  m->p = h;
  const GridP &g = h->g;
  if (g.nx < 2 || g.ny < 2 || g.nz < 2) return FL_ERR_SUP;  // the one-sided wall rows reach two cells inwards
  const int64_t lo[3] = {h->dec.lo[0], h->dec.lo[1], h->dec.lo[2]};
  const int     len[3] = {g.nx, g.ny, g.nz};
  for (int d = 0; d < 3; ++d) {
    std::vector<double> tab, loc;
    FL_CHK(build_axis_momentum(h->ax[d], tab));
    const int64_t n = h->ax[d].n;
    loc.resize((size_t)MOM_NTAB * len[d]);
    for (int a = 0; a < MOM_NTAB; ++a)
      for (int i = 0; i < len[d]; ++i) loc[(size_t)a * len[d] + i] = tab[(size_t)a * n + (size_t)(lo[d] + i)];
    FL_CHK(mom_upload(h, m->tabs[d], loc, 0));
    m->mp.tab[d] = m->tabs[d];
    m->mp.len[d] = len[d];
    for (int slot = 0; slot < 2; ++slot) FL_CHK(m->stabs[slot][d].plain(h, (int64_t)MOM_STAB * len[d]));
    m->mp.stab[d] = m->stabs[0][d];
    // interpolation rows of the owned faces
    const int nfl = d == 0 ? g.fx : (d == 1 ? g.fy : g.fz);
    std::vector<double> bw((size_t)4 * nfl, 0.);
    for (int kind = 0; kind < 3; ++kind) {
      std::vector<double> w0, w1;
      std::vector<int>    c0;
      FL_CHK(build_axis_faceinterp(h->ax[d], kind, w0, w1, c0));
      std::vector<double> l0(nfl), l1(nfl);
      std::vector<int>    lc(nfl);
      for (int f = 0; f < nfl; ++f) {
        l0[f] = w0[(size_t)(lo[d] + f)];
        l1[f] = w1[(size_t)(lo[d] + f)];
        lc[f] = (int)(c0[(size_t)(lo[d] + f)] - lo[d]);
        if (kind >= 1) {
          bw[(size_t)4 * f + 2 * (kind - 1)]     = l0[f];
          bw[(size_t)4 * f + 2 * (kind - 1) + 1] = l1[f];
        }
      }
      FL_CHK(mom_upload(h, m->tw0[kind][d], l0, 1));  // (8 bytes at the least)
      FL_CHK(mom_upload(h, m->tw1[kind][d], l1, 1));
      FL_CHK(mom_upload(h, m->tc0[kind][d], lc, 2));
      m->ft.w0[kind][d] = m->tw0[kind][d];
      m->ft.w1[kind][d] = m->tw1[kind][d];
      m->ft.c0[kind][d] = m->tc0[kind][d];
    }
    FL_CHK(mom_upload(h, m->bws[d], bw, 4));
    m->mp.bw[d] = m->bws[d];
  }
  m->mp.cI = 1.;
  m->mp.cC = 0.;
  m->mp.cL = 0.;
  const MomPlan pl = mom_plan(g);
  if (pl.t2blocks > MAX_PARTIAL_BLOCKS) return FL_ERR_SUP;
  m->t2x      = pl.t2x;
  m->t2chunk  = pl.t2chunk;
  m->t2zc     = pl.t2zc;
  m->t2blocks = pl.t2blocks;
  FL_CHK(fl_ensure_partials(h, m->t2blocks));
  FL_CHK(m->F.exact(h, 12 * (int64_t)h->padlen, true));
  FL_CHK(m->dg.exact(h, 3 * (int64_t)h->padlen, true));
  return fl_momentum_set_coefficients(m, 1., 0., 0.);  // A = I until the first set_state (also fills diag(A))
}

}  // namespace

extern "C" int fl_momentum_create(fl_poisson *grid_from, fl_momentum **out)
{
  if (!grid_from || !out) return FL_ERR_ARG_NULL;
  *out = nullptr;
  FL_HIP(hipSetDevice(grid_from->device));
  fl_momentum *m = new (std::nothrow) fl_momentum;
  if (!m) return FL_ERR_MEM;
  const int rc = mom_init(m, grid_from);
  if (rc != 0) {
    fl_momentum_destroy(m);
    return rc;
  }
  *out = m;
  return FL_SUCCESS;
}

extern "C" int fl_momentum_destroy(fl_momentum *m)
{
  if (!m) return FL_SUCCESS;
  if (m->p) {
    (void)hipSetDevice(m->p->device);
    (void)hipStreamSynchronize(m->p->stream);
  }
  delete m;  // the DevBufs free what they hold
  return FL_SUCCESS;
}

extern "C" int fl_momentum_set_coefficients(fl_momentum *m, double cI, double cC, double cL)
{
  if (!m) return FL_ERR_ARG_NULL;
  m->mp.cI = cI;
  m->mp.cC = cC;
  m->mp.cL = cL;
  m->gersh = -1.;
  fl_poisson *h = m->p;
  FL_HIP(hipSetDevice(h->device));
  FL_CHK(mom_scale_tables(m, 0, m->mp));
  mom_apply_t<0, false, 2>(m, m->F, m->dg, nullptr, nullptr);  // x is not used for the diagonal: any valid padded array
  FL_HIP(hipGetLastError());
  return FL_SUCCESS;
}

namespace {
int mom_set_state(fl_momentum *m, double dt, double rho, double mu, const double *const V0_dev[3], const double *const v0interp_dev[9], const double *v0_dev)
{
  if (!m || !V0_dev || !v0interp_dev) return FL_ERR_ARG_NULL;
  if (!(rho > 0.)) return FL_ERR_ARG_OUTOFRANGE;
  fl_poisson  *h = m->p;
  const GridP &g = h->g;
  FL_HIP(hipSetDevice(h->device));
  for (int d = 0; d < 3; ++d) {
    if (!V0_dev[d]) return FL_ERR_ARG_NULL;
    for (int c = 0; c < 3; ++c)
      if (!v0interp_dev[c * 3 + d]) return FL_ERR_ARG_NULL;
  }
  const int ext[3][3] = {{g.fx, g.ny, g.nz}, {g.nx, g.fy, g.nz}, {g.nx, g.ny, g.fz}};
  // with v0 handed over and k_mom3 certain to run (see mom_apply_t), the inner faces of the nine stored v0interp fields are never read: only their
  // block-end faces are copied (grids with ny <= 8 read the whole fields through k_mom2 and get whole copies)
  const bool ends_only = v0_dev && mom3_grid(g);
  for (int f = 0; f < 12; ++f) {
    const int     d = f < 3 ? f : (f - 3) % 3;
    const double *src = f < 3 ? V0_dev[f] : v0interp_dev[f - 3];
    double       *dst = m->F + (size_t)f * h->padlen;
    const int64_t n = (int64_t)ext[d][0] * ext[d][1] * ext[d][2];
    if (f >= 3 && ends_only)  // k_mom3 reads a stored v0interp field on the block-end faces only
      hipLaunchKernelGGL(k_pad_copy_ends, dim3(nblk_flat(2 * n / std::max(ext[d][d], 1))), dim3(256), 0, h->stream, g, src, dst, ext[d][0], ext[d][1], ext[d][2], d);
    else hipLaunchKernelGGL(k_pad_copy_ext, dim3(nblk_flat(n)), dim3(256), 0, h->stream, g, src, dst, ext[d][0], ext[d][1], ext[d][2]);
    // high face of the last owned cell: periodic image or the neighbour's first face (the physical last face came with the copy)
    if (fl_any_ghost_exchange(h)) FL_CHK(fl_fill_ghosts(h, dst));
  }
  m->fly = false;
  if (v0_dev) {
    FL_CHK(m->v0p.once(h, 3 * (int64_t)h->padlen, true));
    for (int c = 0; c < 3; ++c) launch_pad_copy(h->stream, g, v0_dev + (size_t)c * h->ncell, m->v0p + (size_t)c * h->padlen);
    FL_CHK(mom_ghosts(m, m->v0p));
    m->fly = true;
  }
  m->have_state = true;
  return fl_momentum_set_coefficients(m, 1., dt, -0.5 * mu * dt / rho);  // MatScale(A, dt); MatAXPY(A, -mu dt / 2 rho, L); MatShift(A, 1)
}
}  // namespace

extern "C" int fl_momentum_set_state(fl_momentum *m, double dt, double rho, double mu, const double *const V0_dev[3], const double *const v0interp_dev[9])
{
  return mom_set_state(m, dt, rho, mu, V0_dev, v0interp_dev, nullptr);
}

// The same state, with the cell-centred v0 that v0interp was interpolated from (v0interp = B v0 + vbc, cnlinearcart3d.c:2826-2829; vbc
// lives on boundary faces only): the operator then reads v0interp only on the faces at the ends of this rank's block and forms the
// inner ones from v0 (k_mom3: 96 B/cell per product instead of 144).
extern "C" int fl_momentum_set_state_v0(fl_momentum *m, double dt, double rho, double mu, const double *const V0_dev[3], const double *const v0interp_dev[9], const double *v0_dev)
{
  if (!v0_dev) return FL_ERR_ARG_NULL;
  return mom_set_state(m, dt, rho, mu, V0_dev, v0interp_dev, v0_dev);
}

extern "C" int fl_momentum_apply(fl_momentum *m, const double *v_dev, double *y_dev)
{
  if (!m || !v_dev || !y_dev) return FL_ERR_ARG_NULL;
  if (!m->have_state && m->mp.cC != 0.) return FL_ERR_ARG_WRONGSTATE;
  fl_poisson *h = m->p;
  FL_HIP(hipSetDevice(h->device));
  FL_CHK(mom_stage(m, v_dev));
  mom_apply_t<0, false, 1>(m, m->vec[7], y_dev, nullptr, nullptr);
  FL_HIP(hipGetLastError());
  return FL_SUCCESS;
}

extern "C" int fl_momentum_diagonal(fl_momentum *m, double *d_dev)
{
  if (!m || !d_dev) return FL_ERR_ARG_NULL;
  if (!m->have_state && m->mp.cC != 0.) return FL_ERR_ARG_WRONGSTATE;
  fl_poisson *h = m->p;
  FL_HIP(hipSetDevice(h->device));
  mom_apply_t<0, false, 2>(m, m->F, m->dg, nullptr, nullptr);
  for (int c = 0; c < 3; ++c) launch_unpad_copy(h->stream, h->g, m->dg + (size_t)c * h->padlen, d_dev + (size_t)c * h->ncell, nullptr);
  FL_HIP(hipGetLastError());
  return FL_SUCCESS;
}

// MatGetRowSum(A): A applied to the vector of ones (couplings between the components included)
extern "C" int fl_momentum_rowsum(fl_momentum *m, double *out_dev)
{
  if (!m || !out_dev) return FL_ERR_ARG_NULL;
  if (!m->have_state && m->mp.cC != 0.) return FL_ERR_ARG_WRONGSTATE;
  fl_poisson   *h = m->p;
  const int64_t n3 = 3 * h->ncell;
  FL_HIP(hipSetDevice(h->device));
  FL_CHK(m->tmpv.once(h, n3, true));
  hipLaunchKernelGGL(k_fill, dim3(nblk_flat(n3)), dim3(256), 0, h->stream, n3, 1., m->tmpv.p);
  return fl_momentum_apply(m, m->tmpv, out_dev);
}

// max of a and sum of b over the owned cells (all ranks) of three padded components each: set-up quantities, one launch and one host wait for both
static int max_sum_owned(fl_momentum *m, const double *a3, const double *b3, double *mx_out, double *sum_out)
{
  fl_poisson   *h = m->p;
  const int64_t rows = (int64_t)3 * h->g.nz * h->g.ny;
  const int     nb = (int)std::max<int64_t>(1, std::min<int64_t>((rows + 3) / 4, 2048));
  FL_CHK(fl_ensure_partials(h, 2 * nb));
  hipLaunchKernelGGL(k_max_sum_owned, dim3(nb), dim3(256), 0, h->stream, h->g, (int64_t)h->padlen, a3, b3, h->partial);
  FL_HIP(hipGetLastError());
  std::vector<double> part((size_t)(2 * nb));
  FL_HIP(hipMemcpyAsync(part.data(), h->partial, sizeof(double) * (size_t)(2 * nb), hipMemcpyDeviceToHost, h->stream));
  FL_HIP(hipStreamSynchronize(h->stream));
  double mx = 0., sm = 0.;
  for (int q = 0; q < nb; ++q) {  // fixed order: the same numbers run to run
    mx = std::max(mx, part[(size_t)(2 * q)]);
    sm += part[(size_t)(2 * q + 1)];
  }
  FL_CHK(fl_allreduce_max(h, &mx));  // several ranks: the bound of the whole operator
  FL_CHK(fl_allreduce_sum(h, &sm));
  if (mx_out) *mx_out = mx;
  if (sum_out) *sum_out = sm;
  return 0;
}

// Gershgorin radius of the Jacobi-scaled operator: max_i (sum_{j != i} |a_ij|) / |a_ii|, the entries taken from the same row
// coefficients the product multiplies with (k_mom2 / k_mom3, OUT == 3).  Every eigenvalue of D^-1 A lies in the disc |lambda - 1| <= radius.
// One product-sized launch and one host wait per state; cached until the state or the coefficients change.
extern "C" int fl_momentum_gershgorin(fl_momentum *m, double *radius)
{
  if (!m || !radius) return FL_ERR_ARG_NULL;
  if (!m->have_state && m->mp.cC != 0.) return FL_ERR_ARG_WRONGSTATE;
  fl_poisson *h = m->p;
  FL_HIP(hipSetDevice(h->device));
  if (m->gersh < 0.) {
    FL_CHK(mom_vec(m, 7));
    mom_apply_t<0, false, 3>(m, m->F, m->vec[7], nullptr, nullptr);  // x is not used for the row sums: any valid padded array
    double dsum = 0.;
    FL_CHK(max_sum_owned(m, m->vec[7], m->dg, &m->gersh, &dsum));
    m->dmean = dsum / (3. * (double)h->ax[0].n * (double)h->ax[1].n * (double)h->ax[2].n);
  }
  *radius = m->gersh;
  return FL_SUCCESS;
}

// The interval KSPCHEBYSHEV on kspA uses when none is given (PCJACOBI): emax = 1 + g from the Gershgorin disc of D^-1 A (a bound), emin = the
// larger of 1 - g (the disc again, while the operator is diagonally dominant) and 0.9 / mean_i a_ii.  Why the mean: with E = dt C - (mu dt /
// 2 rho) L of non-negative symmetric part (a skew convection operator, a symmetric negative Laplacian) the Rayleigh quotient of
// D^-1/2 A D^-1/2 is (x.x + x.E x) / (x.D x) >= x.x / x.D x, and the vectors that make x.E x small are the smooth ones, for which x.D x / x.x
// is the MEAN diagonal entry -- 1 / max a_ii, the rigorous bound, is decided by the wall rows (twice the interior diagonal) and costs half
// again as many steps: a 32^3 channel at nu dt / h^2 = 2.56 has lambda_min = 0.1188, 1 / mean = 0.112, 1 / max = 0.061; 24 steps with
// the true interval, 27 with this rule, 37 with 1 / max (profiles/r04_mom_cheb.txt).  An emin above the true one slows the lowest modes
// down, it does not break the iteration.
extern "C" int fl_momentum_chebyshev_interval(fl_momentum *m, double *emin, double *emax)
{
  if (!m || !emin || !emax) return FL_ERR_ARG_NULL;
  double g = 0.;
  FL_CHK(fl_momentum_gershgorin(m, &g));
  *emax = 1. + g;
  *emin = std::max(1. - g, 0.9 / m->dmean);
  return FL_SUCCESS;
}

// The part of momrhs (NSFormFunction_CNLinear_Cart3d_Internal, cnlinearcart3d.c:2976-2998) that lives on every cell:
//   momrhs = v0 + (mu dt / 2 rho) L v0 - kappa G p  (+ vbc: the boundary-condition vectors, combined by the caller)
extern "C" int fl_momentum_rhs(fl_momentum *m, double dt, double rho, double mu, const double *v0_dev, const double *p_dev, const double *vbc_dev, double *momrhs_dev)
{
  if (!m || !v0_dev || !momrhs_dev) return FL_ERR_ARG_NULL;
  if (!(rho > 0.)) return FL_ERR_ARG_OUTOFRANGE;
  fl_poisson *h = m->p;
  FL_HIP(hipSetDevice(h->device));
  const size_t N = (size_t)h->ncell;
  FL_CHK(mom_stage(m, v0_dev));
  MomP co = m->mp;
  co.cI   = 1.;
  co.cC   = 0.;
  co.cL   = 0.5 * mu * dt / rho;  // VecAXPBYPCZ(momrhs, 1, mu dt / 2 rho, 0, v0, Lv), :2988
  FL_CHK(mom_scale_tables(m, 1, co));
  mom_apply_t<0, false, 1>(m, m->vec[7], momrhs_dev, nullptr, nullptr, &co);
  if (p_dev) FL_CHK(fl_poisson_project(h, p_dev, momrhs_dev, momrhs_dev + N, momrhs_dev + 2 * N, nullptr, nullptr, nullptr));  // VecAXPY(momrhs, -1, Gp), :2993
  if (vbc_dev) lincomb(h, (int64_t)(3 * N), 1., momrhs_dev, 1., vbc_dev, momrhs_dev);
  FL_HIP(hipGetLastError());
  return FL_SUCCESS;
}

// ------------------------------------------------------------------------------------------------ diagnostics

// the operator kernel alone on padded work vectors (no pad / unpad copies): mode 0 plain, 1 Jacobi, 2 Jacobi + y.o (the first product of a
// BiCGStab iteration), 3 Jacobi + x.y, y.y (the second)
extern "C" int fldbg_mom_apply(fl_momentum *m, int mode, int reps, double *ms_out)
{
  fl_poisson *h = m->p;
  FL_HIP(hipSetDevice(h->device));
  FL_CHK(mom_vec(m, 5));
  FL_CHK(mom_vec(m, 6));
  FL_CHK(mom_vec(m, 7));
  auto go = [&]() {
    switch (mode & 3) {
      case 0: mom_apply_t<0, false, 0>(m, m->vec[7], m->vec[6], nullptr, nullptr); break;
      case 1: mom_apply_t<0, true, 0>(m, m->vec[7], m->vec[6], nullptr, nullptr); break;
      case 2: mom_apply_t<1, true, 0>(m, m->vec[7], m->vec[6], m->vec[5], nullptr); break;
      default: mom_apply_t<2, true, 0>(m, m->vec[7], m->vec[6], nullptr, nullptr); break;
    }
  };
  go();
  FL_HIP(hipEventRecord(h->ev0, h->stream));
  for (int r = 0; r < reps; ++r) go();
  FL_HIP(hipEventRecord(h->ev1, h->stream));
  FL_HIP(hipStreamSynchronize(h->stream));
  FL_HIP(hipGetLastError());
  float ms = 0.f;
  FL_HIP(hipEventElapsedTime(&ms, h->ev0, h->ev1));
  *ms_out = ms / reps;
  return 0;
}
