// fl_scalar_implicit.hip -- implicit diffusion of the passive scalar (include/fluca_hip_implicit.h): the Helmholtz operator H_c(phi) = phi - c D(phi) of the
// two-point diffusion term of fl_scalar.hip, D(phi)(c) = sum_d [ g_d(f+) - g_d(f-) ] / h_d(c) with sc_axis's boundary rule (what k_scalar_stage forms with
// V = 0, Gamma = 1, q = 0), its solve by Chebyshev-Jacobi on a Gershgorin interval, and the IMEX step: the explicit stages of fl_scalar_step without the
// diffusion term, then the solve.  DESIGN.md section 4 has the interval, the norm of the bound and what theta means.
//
// A = I - c L is strictly diagonally dominant, so the spectrum of diag^-1 A lies in [1 / (1 + S), (1 + 2 S) / (1 + S)], S = c sum_d max_i omega_d(i), which
// the host knows from the 1-D tables: the step count for a given reduction of the error is fixed BEFORE the first launch, the coefficients of every step
// (the three-term recurrence of Saad's Algorithm 12.1, which k_cheb_st follows as well) are formed on the host in double and travel as kernel arguments,
// and nothing here reduces, fetches or waits: a solve is k launches.
//
// k_scalar_cheb, one step per launch:  r = b - H_c(x);  d' = p d + q r / diag;  x' = x + d'.  7-point star on the caller's UNPADDED array, read as
// k_scalar_stage reads w (sc_ld: a cell outside the line is its periodic image or is replaced by the boundary rule, in registers); the diagonal is formed
// from the cell's three table rows -- no diagonal array, no padded copy.  d in place, x' into the other x array.  x 8 + b 8 + d 8 read, x' 8 + d' 8
// written = 40 B/cell (32 in the first step, which does not read d).  The sweep is k_scalar_stage's: XCD-banded rows, a wave keeps one x segment when the
// launch allows it, b and d non-temporal.  No velocities and no limiter: 8 waves a SIMD (profiles/scalar_implicit_devcode.txt), no scratch.
//
// Several ranks (include/fluca_hip_implicit_ranks.h, k_scalar_cheb_ring): the same sweep over the rank's block.  The star reaches one cell across a rank face, so
// ONE plane per face travels per step, through the slabs and the message plan of fl_scalar.hip (scalar_ring_exchange1); a step that is not the last also stores
// the cells it writes next to a rank face into the send layers, so one exchange and one launch stand between two steps.  The interval is that of the GLOBAL
// tables on every rank: the same count everywhere, no vote, no reduction -- and, cell for cell, the operations and operands of the one-rank kernel: the gathered
// result has its bits.  The exchange is not overlapped with the sweep (fl_scalar.hip's decision for the stages, for the same reason).
#include "fl_device.h"
#include "fl_handle.h"
#include "fl_scalar_handle.h"
#include "../../include/fluca_hip_implicit.h"
#include "../../include/fluca_hip_implicit_ranks.h"

namespace fl {

// The contribution of one axis to D at cell a of a line, and to the diagonal of -L (dg).  ic1 / ic2: 1 / distance of the faces a / a+1, ih: 1 / width.
// The gradients are sc_axis's G1, G2 with its boundary rule; a face adds its ic to the diagonal where phi_a enters its gradient with a partner: an interior or
// periodic face (not the face of a one-cell periodic axis, whose partner is the cell itself) and a Dirichlet face.
// RING (k_scalar_cheb_ring): behind an end with a neighbouring rank the cell -1 / n comes from the slabs of e, and that end is no physical boundary -- its
// face is an interior face, its ic on the diagonal.  Only the two loads and the predicates lo0 / hi0 differ; the arithmetic is this one piece of source.
template <bool RING>
__device__ __forceinline__ double hc_axis(double ic1, double ic2, double ih, const double *__restrict__ x, double P2, int a, int n, bool wraps, int klo, int khi, double vlo, double vhi, int64_t c0,
                                          int64_t cs, const ScEnds &e, double &dg)
{
  double Pm, Pp;
  bool   lo0, hi0;
  if constexpr (RING) {
    Pm = sc_ld_ring(x, c0, cs, a - 1, n, wraps, e), Pp = sc_ld_ring(x, c0, cs, a + 1, n, wraps, e);
    lo0 = !wraps && !e.nlo && a == 0, hi0 = !wraps && !e.nhi && a == n - 1;
  } else {
    Pm = sc_ld(x, c0, cs, a - 1, n, wraps), Pp = sc_ld(x, c0, cs, a + 1, n, wraps);
    lo0 = !wraps && a == 0, hi0 = !wraps && a == n - 1;
  }
  const bool self = wraps && n == 1;
  if (klo == 0 && lo0) Pm = vlo;
  if (khi == 0 && hi0) Pp = vhi;
  double G1 = (P2 - Pm) * ic1, G2 = (Pp - P2) * ic2;
  if (klo == 1 && lo0) G1 = vlo;
  if (khi == 1 && hi0) G2 = vhi;
  const double w1 = (self || (lo0 && klo == 1)) ? 0. : ic1, w2 = (self || (hi0 && khi == 1)) ? 0. : ic2;
  dg += (w1 + w2) * ih;
  return (G2 - G1) * ih;
}

// MODE 0: a Chebyshev step; 1: the first step (d is not read); 2: out = H_c(x) (xo; b and d not used); 3: out = -c D(x) (the explicit share of the diffusion
// of a theta < 1 step, with c < 0).  Grid: a multiple of 8 blocks; block b works for XCD b % 8 on the y band of it (k_scalar_stage).
constexpr int HC_WAVES = 8;  // waves a SIMD = blocks of 256 a CU
template <int MODE>
__global__ void __launch_bounds__(256, HC_WAVES) k_scalar_cheb(ScGrid g, double cc, double p, double q, const double *__restrict__ x, const double *__restrict__ b, double *__restrict__ d,
                                                              double *__restrict__ xo)
{
  const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), nw = blockDim.x >> 6;
  const int xcd = blockIdx.x & 7, lb = blockIdx.x >> 3, nlb = gridDim.x >> 3;
  const int band = (g.ny + 7) / 8, j0 = xcd * band, j1 = min(j0 + band, g.ny);
  if (j0 >= j1) return;
  const int     nseg = (g.nx + 63) / 64, nj = j1 - j0;
  const int64_t nitem = (int64_t)nseg * nj * g.nz, nxy = (int64_t)g.nx * g.ny;
  const bool    wx = g.per & 1, wy = g.per & 2, wz = g.per & 4;
  // a wave keeps ONE x segment for all its rows whenever the launch allows it: the x numbers of its cells are fetched once
  const bool   fixed_seg = ((int64_t)nlb * nw) % nseg == 0;
  const int    seg0 = (int)(((int64_t)lb * nw + wv) % nseg), i0 = min(seg0 * 64 + lane, g.nx - 1);
  const double xa0 = g.c[0][i0].ic1, xb0 = g.c[0][i0].ic2, xh0 = g.c[0][i0].ih;
  const ScEnds none = {false, false, nullptr, 0, 0};  // (one rank: not read)
  for (int64_t it = (int64_t)lb * nw + wv; it < nitem; it += (int64_t)nlb * nw) {
    const int seg = (int)(it % nseg), row = (int)(it / nseg);
    const int j = j0 + row % nj, k = row / nj, i = seg * 64 + lane;
    if (i >= g.nx) continue;
    const int64_t urow = ((int64_t)k * g.ny + j) * g.nx, c = urow + i;
    const ScCell &TX = g.c[0][i], &TY = g.c[1][j], &TZ = g.c[2][k];
    const double  P2 = x[c];
    double        dg = 0.;
    double        D = hc_axis<false>(fixed_seg ? xa0 : TX.ic1, fixed_seg ? xb0 : TX.ic2, fixed_seg ? xh0 : TX.ih, x, P2, i, g.nx, wx, g.kind[0], g.kind[1], g.val[0], g.val[1], urow, 1, none, dg);
    D += hc_axis<false>(TY.ic1, TY.ic2, TY.ih, x, P2, j, g.ny, wy, g.kind[2], g.kind[3], g.val[2], g.val[3], (int64_t)k * nxy + i, g.nx, none, dg);
    D += hc_axis<false>(TZ.ic1, TZ.ic2, TZ.ih, x, P2, k, g.nz, wz, g.kind[4], g.kind[5], g.val[4], g.val[5], (int64_t)j * g.nx + i, nxy, none, dg);
    if (MODE == 2) {
      __builtin_nontemporal_store(P2 - cc * D, xo + c);
    } else if (MODE == 3) {
      __builtin_nontemporal_store(-(cc * D), xo + c);
    } else {
      const double r = __builtin_nontemporal_load(b + c) - (P2 - cc * D);
      double       dn = q * (r / (1. + cc * dg));
      if (MODE == 0) dn += p * __builtin_nontemporal_load(d + c);
      __builtin_nontemporal_store(dn, d + c);
      xo[c] = P2 + dn;  // (the next step reads it through the star: not non-temporal)
    }
  }
}

// What a rank's block of several reads and writes beside its own arrays (wave-uniform: scalar registers): the handle's slabs (ScRing of fl_scalar.hip; of an
// axis's four layers this star reads the receive layers 1, 2 -- the cells -1, n -- and fills the send layers 0, 3 -- the cells 0, n - 1).  nb: bit 2 d / 2 d + 1
// = a neighbouring rank behind the low / high end of axis d.  pack: the boundaries (bits as nb) whose send layer this step fills with x' -- 0 in the last step
// of a solve and in the modes 2, 3.
struct HcRing {
  const double *recv;
  double       *send;
  int           nb, pack;
};

// k_scalar_cheb on one rank's block of several: the same sweep, plan, modes and arithmetic; g: the block (per: the periodic axes the rank holds alone), the
// tables cut to its rows, so a cell runs the operations of the one-rank kernel on its operands.
template <int MODE>
__global__ void __launch_bounds__(256, HC_WAVES) k_scalar_cheb_ring(ScGrid g, HcRing rg, double cc, double p, double q, const double *__restrict__ x, const double *__restrict__ b,
                                                                   double *__restrict__ d, double *__restrict__ xo)
{
  const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), nw = blockDim.x >> 6;
  const int xcd = blockIdx.x & 7, lb = blockIdx.x >> 3, nlb = gridDim.x >> 3;
  const int band = (g.ny + 7) / 8, j0 = xcd * band, j1 = min(j0 + band, g.ny);
  if (j0 >= j1) return;
  const int     nseg = (g.nx + 63) / 64, nj = j1 - j0;
  const int64_t nitem = (int64_t)nseg * nj * g.nz, nxy = (int64_t)g.nx * g.ny, nyz = (int64_t)g.ny * g.nz, nxz = (int64_t)g.nx * g.nz;
  const bool    wx = g.per & 1, wy = g.per & 2, wz = g.per & 4;
  const bool    lx = rg.nb & 1, hx = rg.nb & 2, ly = rg.nb & 4, hy = rg.nb & 8, lz = rg.nb & 16, hz = rg.nb & 32;
  const bool    fixed_seg = ((int64_t)nlb * nw) % nseg == 0;
  const int     seg0 = (int)(((int64_t)lb * nw + wv) % nseg), i0 = min(seg0 * 64 + lane, g.nx - 1);
  const double  xa0 = g.c[0][i0].ic1, xb0 = g.c[0][i0].ic2, xh0 = g.c[0][i0].ih;
  for (int64_t it = (int64_t)lb * nw + wv; it < nitem; it += (int64_t)nlb * nw) {
    const int seg = (int)(it % nseg), row = (int)(it / nseg);
    const int j = j0 + row % nj, k = row / nj, i = seg * 64 + lane;
    if (i >= g.nx) continue;
    const int64_t prx = (int64_t)k * g.ny + j, pry = (int64_t)k * g.nx + i, prz = (int64_t)j * g.nx + i;  // this cell's line in the planes across x / y / z
    const int64_t urow = prx * g.nx, c = urow + i;
    const ScCell &TX = g.c[0][i], &TY = g.c[1][j], &TZ = g.c[2][k];
    const double  P2 = x[c];
    double        dg = 0.;
    double        D = hc_axis<true>(fixed_seg ? xa0 : TX.ic1, fixed_seg ? xb0 : TX.ic2, fixed_seg ? xh0 : TX.ih, x, P2, i, g.nx, wx, g.kind[0], g.kind[1], g.val[0], g.val[1], urow, 1,
                                    ScEnds{lx, hx, rg.recv, nyz, prx}, dg);
    D += hc_axis<true>(TY.ic1, TY.ic2, TY.ih, x, P2, j, g.ny, wy, g.kind[2], g.kind[3], g.val[2], g.val[3], (int64_t)k * nxy + i, g.nx, ScEnds{ly, hy, rg.recv + 4 * nyz, nxz, pry}, dg);
    D += hc_axis<true>(TZ.ic1, TZ.ic2, TZ.ih, x, P2, k, g.nz, wz, g.kind[4], g.kind[5], g.val[4], g.val[5], prz, nxy, ScEnds{lz, hz, rg.recv + 4 * (nyz + nxz), nxy, prz}, dg);
    if (MODE == 2) {
      __builtin_nontemporal_store(P2 - cc * D, xo + c);
    } else if (MODE == 3) {
      __builtin_nontemporal_store(-(cc * D), xo + c);
    } else {
      const double r = __builtin_nontemporal_load(b + c) - (P2 - cc * D);
      double       dn = q * (r / (1. + cc * dg));
      if (MODE == 0) dn += p * __builtin_nontemporal_load(d + c);
      __builtin_nontemporal_store(dn, d + c);
      const double xn = P2 + dn;
      xo[c] = xn;
      // the fused pack: the next step's exchange sends these layers as they are
      if (rg.pack) {
        double *const sx = rg.send, *const sy = sx + 4 * nyz, *const sz = sy + 4 * nxz;
        if ((rg.pack & 1) && i == 0) sx[prx] = xn;
        if ((rg.pack & 2) && i == g.nx - 1) sx[3 * nyz + prx] = xn;
        if ((rg.pack & 4) && j == 0) sy[pry] = xn;
        if ((rg.pack & 8) && j == g.ny - 1) sy[3 * nxz + pry] = xn;
        if ((rg.pack & 16) && k == 0) sz[prz] = xn;
        if ((rg.pack & 32) && k == g.nz - 1) sz[3 * nxy + prz] = xn;
      }
    }
  }
}

// b += x: the second of the two passes that form the right-hand side of a theta < 1 step
__global__ void __launch_bounds__(256) k_scalar_addto(int64_t n, const double *__restrict__ x, double *__restrict__ b)
{
  for (int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x; c < n; c += (int64_t)gridDim.x * 256) b[c] += x[c];
}

}  // namespace fl

using namespace fl;

// ------------------------------------------------------------------------------------------------ host arithmetic: the step count, the interval

extern "C" int fl_scalar_cheb_steps(double emin, double emax, double rtol, int maxit, int *steps, double *bound)
{
  if (!steps || !bound) return FL_ERR_ARG_NULL;
  if (!std::isfinite(emin) || !std::isfinite(emax) || !(emin > 0.) || !(emax >= emin) || !(rtol > 0.) || !(rtol < 1.) || maxit < 0) return FL_ERR_ARG_OUTOFRANGE;
  const int    cap = maxit - maxit % 2;
  const double sk = std::sqrt(emax / emin), sigma = (sk - 1.) / (sk + 1.), s2 = sigma * sigma;
  // B_k = 2 s^k / (1 + s^2k) at k = 2, 4, ...: s^k by repeated products with s^2 (tests/scalar_implicit_reference.py forms the same products)
  int    k = 0;
  double pw = 1., B = 1.;
  while (B > rtol && k < cap) {
    k += 2;
    pw *= s2;
    B = 2. * pw / (1. + pw * pw);
  }
  *steps = k;
  *bound = B;
  return FL_SUCCESS;
}

namespace {

// the plan of k_scalar_cheb: scalar_plan of fl_scalar.hip with this kernel's residency (HC_WAVES blocks on each of an XCD's 32 CUs)
struct ChebPlan {
  int     per_xcd, nseg, band, fixed_seg;
  int64_t items;
};
ChebPlan cheb_plan(int nx, int ny, int nz)
{
  ChebPlan pl;
  pl.nseg      = (nx + 63) / 64;
  pl.band      = (ny + 7) / 8;
  pl.items     = (int64_t)pl.nseg * ny * nz;
  pl.per_xcd   = (int)std::max<int64_t>(1, std::min<int64_t>((pl.items / 8 + 3) / 4, 32 * HC_WAVES));
  pl.fixed_seg = ((int64_t)pl.per_xcd * 4) % pl.nseg == 0 ? 1 : 0;
  return pl;
}

// max_i omega_d(i) for the three axes, from the rows the kernels read: omega_d(i) = ih_i (ic of the faces i and i + 1 that have a cell on the other side)
int implicit_omega(fl_scalar *m)
{
  if (m->have_omega) return FL_SUCCESS;
  for (int d = 0; d < 3; ++d) {
    const Axis         &A = m->h->ax[d];
    std::vector<ScCell> rows;
    FL_CHK(build_axis_scalar(A, rows));
    double most = 0.;
    for (int64_t i = 0; i < A.n; ++i) {
      const ScCell &T  = rows[(size_t)i];
      const double  w1 = (A.periodic ? A.n > 1 : i > 0) ? T.ic1 : 0., w2 = (A.periodic ? A.n > 1 : i + 1 < A.n) ? T.ic2 : 0.;
      most = std::max(most, (w1 + w2) * T.ih);
    }
    m->omega[d] = most;
  }
  m->have_omega = true;
  return FL_SUCCESS;
}

int implicit_interval(fl_scalar *m, double c, double *emin, double *emax, double *S_out)
{
  FL_CHK(implicit_omega(m));
  const double S = c * ((m->omega[0] + m->omega[1]) + m->omega[2]);
  if (!std::isfinite(S)) return FL_ERR_ARG_OUTOFRANGE;
  *emin = 1. / (1. + S);
  *emax = (1. + 2. * S) / (1. + S);
  if (S_out) *S_out = S;
  return FL_SUCCESS;
}

// pack (several ranks, modes 0 and 1): the step also fills the send layers with x', for the exchange of the step after it
template <int MODE>
void launch_cheb(const fl_scalar *m, double c, double p, double q, const double *x, const double *b, double *d, double *xo, bool pack = false)
{
  const dim3 grid(8 * cheb_plan(m->g.nx, m->g.ny, m->g.nz).per_xcd);
  if (m->ring) {
    const HcRing rg = {m->slab_recv.p, m->slab_send.p, m->nb, (pack && MODE < 2) ? m->nb : 0};
    hipLaunchKernelGGL((k_scalar_cheb_ring<MODE>), grid, dim3(256), 0, m->h->stream, m->g, rg, c, p, q, x, b, d, xo);
    return;
  }
  hipLaunchKernelGGL((k_scalar_cheb<MODE>), grid, dim3(256), 0, m->h->stream, m->g, c, p, q, x, b, d, xo);
}

int implicit_arrays(fl_scalar *m, bool with_b)
{
  for (int a = 0; a < 2; ++a)
    if (!m->work[a]) FL_CHK(m->work[a].plain(m->h, m->h->ncell));
  if (with_b && !m->imex_b) FL_CHK(m->imex_b.plain(m->h, m->h->ncell));
  return FL_SUCCESS;
}

// The launches of a solve whose count and interval are known (info): the guess is read from x0 (x_dev itself, or b_dev where the guess IS b), step 1 writes
// the handle's other iterate, step 2 x_dev, and so on: an even count ends in x_dev.  d: work[0], the other iterate: work[1].
//   theta_c = (emax + emin) / 2, delta = (emax - emin) / 2, sigma_1 = theta_c / delta, rho_0 = 1 / sigma_1, d_0 = r_0 / theta_c;
//   rho_j = 1 / (2 sigma_1 - rho_{j-1}), d_j = rho_j rho_{j-1} d_{j-1} + (2 rho_j / delta) r_j             (r: the Jacobi-preconditioned residual)
// Several ranks: the send layers hold the guess's outermost cells when this is called (scalar_ring_pack1, or a stage that packed); every step is one
// one-plane exchange and one launch, and every step but the last fills the send layers with its x'.  The count is host arithmetic on the global tables --
// the same on every rank -- so nothing is voted and nothing reduced.
int cheb_launches(fl_scalar *m, double c, const fl_scalar_cheb_info &info, const double *b, const double *x0, double *x_dev)
{
  const double theta = 0.5 * (info.emax + info.emin), delta = 0.5 * (info.emax - info.emin), sigma1 = theta / delta;
  double       rho = 1. / sigma1;
  double      *d = m->work[0], *other = m->work[1];
  const double *xin = x0;
  for (int j = 1; j <= info.steps; ++j) {
    double    *xout = (j & 1) ? other : x_dev;
    const bool pack = j < info.steps;
    if (m->ring) FL_CHK(scalar_ring_exchange1(m));
    if (j == 1) launch_cheb<1>(m, c, 0., 1. / theta, xin, b, d, xout, pack);
    else {
      const double rho_new = 1. / (2. * sigma1 - rho);
      launch_cheb<0>(m, c, rho_new * rho, 2. * rho_new / delta, xin, b, d, xout, pack);
      rho = rho_new;
    }
    xin = xout;
  }
  FL_HIP(hipGetLastError());
  return FL_SUCCESS;
}

// interval and count of a solve with c; S = 0 (c = 0, or a grid without a face between two cells): nothing to iterate on, steps = 0 and x = b
int cheb_prepare(fl_scalar *m, double c, double rtol, int maxit, fl_scalar_cheb_info *info, double *S)
{
  FL_CHK(implicit_interval(m, c, &info->emin, &info->emax, S));
  info->steps = info->capped = 0;
  info->bound = 1.;
  if (*S == 0.) return FL_SUCCESS;
  FL_CHK(fl_scalar_cheb_steps(info->emin, info->emax, rtol, maxit, &info->steps, &info->bound));
  info->capped = info->bound > rtol ? 1 : 0;
  return FL_SUCCESS;
}

bool bad_c(double c) { return !(c >= 0.) || !std::isfinite(c); }
bool bad_solve_args(double rtol, int maxit) { return !(rtol > 0.) || !(rtol < 1.) || maxit < 0; }

}  // namespace

// Not part of the public C-ABI (tests): the plan of k_scalar_cheb on an nx x ny x nz block, as fldbg_scalar_plan -- 0 per_xcd, 1 nseg, 2 band, 3 fixed_seg, 4 items
extern "C" int fldbg_scalar_cheb_plan(int nx, int ny, int nz, int *out, int nout)
{
  if (nx < 1 || ny < 1 || nz < 1) return FL_ERR_ARG_OUTOFRANGE;
  if (!out) return 5;
  if (nout < 5) return FL_ERR_ARG_SIZ;
  const ChebPlan pl = cheb_plan(nx, ny, nz);
  if (pl.items > INT32_MAX) return FL_ERR_ARG_OUTOFRANGE;
  out[0] = pl.per_xcd; out[1] = pl.nseg; out[2] = pl.band; out[3] = pl.fixed_seg; out[4] = (int)pl.items;
  return 5;
}

// Not part of the public C-ABI (tools/scalar_implicit_bench.py): ONE Chebyshev step with the coefficients p, q -- first != 0: the first step's kernel, which
// does not read d_dev -- from x_dev into xo_dev
extern "C" int fldbg_scalar_cheb_one(fl_scalar *m, double c, double p, double q, int first, const double *x_dev, const double *b_dev, double *d_dev, double *xo_dev)
{
  if (!m || !x_dev || !b_dev || !d_dev || !xo_dev) return FL_ERR_ARG_NULL;
  if (x_dev == xo_dev) return FL_ERR_ARG_WRONG;
  if (m->ring) return FL_ERR_SUP;
  FL_HIP(hipSetDevice(m->h->device));
  if (first) launch_cheb<1>(m, c, p, q, x_dev, b_dev, d_dev, xo_dev);
  else launch_cheb<0>(m, c, p, q, x_dev, b_dev, d_dev, xo_dev);
  FL_HIP(hipGetLastError());
  return FL_SUCCESS;
}

extern "C" int fl_scalar_diffusion_interval(fl_scalar *m, double c, double *emin, double *emax)
{
  if (!m || !emin || !emax) return FL_ERR_ARG_NULL;
  if (bad_c(c)) return FL_ERR_ARG_OUTOFRANGE;
  return implicit_interval(m, c, emin, emax, nullptr);
}

// Not part of the public C-ABI (tools/scalar_implicit_bench.py --ring): fldbg_scalar_cheb_one on a handle of fl_scalar_create_ranks -- ONE launch of
// k_scalar_cheb_ring, no exchange, the slabs as the last collective call left them -- so that one rank can time the kernel while its peers idle.  pack != 0:
// the step also fills the send layers, as every step of a solve but the last does.
extern "C" int fldbg_scalar_cheb_ring_one(fl_scalar *m, double c, double p, double q, int first, int pack, const double *x_dev, const double *b_dev, double *d_dev, double *xo_dev)
{
  if (!m || !x_dev || !b_dev || !d_dev || !xo_dev) return FL_ERR_ARG_NULL;
  if (x_dev == xo_dev) return FL_ERR_ARG_WRONG;
  if (!m->ring) return FL_ERR_SUP;
  FL_HIP(hipSetDevice(m->h->device));
  if (first) launch_cheb<1>(m, c, p, q, x_dev, b_dev, d_dev, xo_dev, pack != 0);
  else launch_cheb<0>(m, c, p, q, x_dev, b_dev, d_dev, xo_dev, pack != 0);
  FL_HIP(hipGetLastError());
  return FL_SUCCESS;
}

namespace {

// The three calls on either kind of handle.  ranks: entered through include/fluca_hip_implicit_ranks.h -- the names of fluca_hip_implicit.h refuse a rank's block
// of several.  On a one-rank handle m->ring is false and every line below that asks for it is skipped: the same launches either way.
int diffusion_apply(fl_scalar *m, double c, const double *phi_dev, double *out_dev, bool ranks)
{
  if (!m || !phi_dev || !out_dev) return FL_ERR_ARG_NULL;
  if (bad_c(c)) return FL_ERR_ARG_OUTOFRANGE;
  if (phi_dev == out_dev) return FL_ERR_ARG_WRONG;  // neighbours still read phi
  if (m->ring && !ranks) return FL_ERR_SUP;
  FL_HIP(hipSetDevice(m->h->device));
  if (m->ring) {
    FL_CHK(scalar_ring_pack1(m, phi_dev));
    FL_CHK(scalar_ring_exchange1(m));
  }
  launch_cheb<2>(m, c, 0., 0., phi_dev, nullptr, nullptr, out_dev);
  FL_HIP(hipGetLastError());
  return FL_SUCCESS;
}

int diffusion_solve(fl_scalar *m, double c, double rtol, int maxit, const double *b_dev, double *x_dev, fl_scalar_cheb_info *info, bool ranks)
{
  if (!m || !b_dev || !x_dev) return FL_ERR_ARG_NULL;
  if (bad_c(c) || bad_solve_args(rtol, maxit)) return FL_ERR_ARG_OUTOFRANGE;
  if (b_dev == x_dev) return FL_ERR_ARG_WRONG;
  if (m->ring && !ranks) return FL_ERR_SUP;
  fl_scalar_cheb_info I;
  double              S = 0.;
  FL_CHK(cheb_prepare(m, c, rtol, maxit, &I, &S));
  FL_HIP(hipSetDevice(m->h->device));
  if (S == 0.) FL_HIP(hipMemcpyAsync(x_dev, b_dev, sizeof(double) * (size_t)m->h->ncell, hipMemcpyDeviceToDevice, m->h->stream));
  else if (I.steps > 0) {
    FL_CHK(implicit_arrays(m, false));
    if (m->ring) FL_CHK(scalar_ring_pack1(m, x_dev));
    FL_CHK(cheb_launches(m, c, I, b_dev, x_dev, x_dev));
  }
  if (info) *info = I;
  return FL_SUCCESS;
}

int step_imex(fl_scalar *m, double dt, int nstages, double theta, double rtol, int maxit, const double *source_dev, double *phi_dev, fl_scalar_cheb_info *info, bool ranks)
{
  if (!m || !phi_dev) return FL_ERR_ARG_NULL;
  if (nstages < 2 || !std::isfinite(dt) || !(dt >= 0.) || !(theta >= 0.5) || !(theta <= 1.) || bad_solve_args(rtol, maxit)) return FL_ERR_ARG_OUTOFRANGE;
  if (m->ring && !ranks) return FL_ERR_SUP;
  if (!m->V[0]) return FL_ERR_ARG_WRONGSTATE;
  const double gamma = m->g.gamma, c = theta * dt * gamma, ce = (1. - theta) * dt * gamma;
  fl_scalar_cheb_info I;
  double              S = 0.;
  FL_CHK(cheb_prepare(m, c, rtol, maxit, &I, &S));
  if (info) *info = I;
  if (gamma == 0.) return scalar_ssp_step(m, dt, nstages, source_dev, phi_dev, phi_dev, false);  // fl_scalar_step, launch for launch and message for message
  FL_HIP(hipSetDevice(m->h->device));
  FL_CHK(implicit_arrays(m, true));
  const size_t ncell = (size_t)m->h->ncell;
  const bool   cn = ce != 0.;
  // theta < 1: the explicit share of the diffusion, from phi^n (before the stages overwrite it)
  if (cn) {
    if (m->ring) {
      FL_CHK(scalar_ring_pack1(m, phi_dev));
      FL_CHK(scalar_ring_exchange1(m));
    }
    launch_cheb<3>(m, -ce, 0., 0., phi_dev, nullptr, nullptr, m->imex_b);
  }
  // The stages with Gamma = 0 (the value travels with each launch).  theta = 1 with steps to run: phi* lands in the right-hand side's array, which is then
  // also the guess -- the first step reads it there, the last writes phi_dev.  Otherwise in place.  Several ranks: that last stage fills the send layers as
  // well, so the first Chebyshev step's exchange follows it with no pack launch in between.
  const bool to_b = !cn && I.steps > 0;
  m->g.gamma = 0.;
  const int rc = scalar_ssp_step(m, dt, nstages, source_dev, phi_dev, to_b ? m->imex_b.p : phi_dev, to_b);
  m->g.gamma = gamma;
  FL_CHK(rc);
  if (to_b) return cheb_launches(m, c, I, m->imex_b, m->imex_b, phi_dev);
  if (!cn) return FL_SUCCESS;  // (no step to run: x = b = the guess = phi*)
  hipLaunchKernelGGL(k_scalar_addto, dim3((unsigned)std::min<size_t>((ncell + 255) / 256, 8192)), dim3(256), 0, m->h->stream, (int64_t)ncell, phi_dev, m->imex_b.p);
  if (S == 0.) FL_HIP(hipMemcpyAsync(phi_dev, m->imex_b, sizeof(double) * ncell, hipMemcpyDeviceToDevice, m->h->stream));
  if (m->ring && I.steps > 0) FL_CHK(scalar_ring_pack1(m, phi_dev));  // the guess phi*
  return cheb_launches(m, c, I, m->imex_b, phi_dev, phi_dev);
}

}  // namespace

extern "C" int fl_scalar_diffusion_apply(fl_scalar *m, double c, const double *phi_dev, double *out_dev) { return diffusion_apply(m, c, phi_dev, out_dev, false); }

extern "C" int fl_scalar_diffusion_solve(fl_scalar *m, double c, double rtol, int maxit, const double *b_dev, double *x_dev, fl_scalar_cheb_info *info)
{
  return diffusion_solve(m, c, rtol, maxit, b_dev, x_dev, info, false);
}

extern "C" int fl_scalar_step_imex(fl_scalar *m, double dt, int nstages, double theta, double rtol, int maxit, const double *source_dev, double *phi_dev,
                                   fl_scalar_cheb_info *info)
{
  return step_imex(m, dt, nstages, theta, rtol, maxit, source_dev, phi_dev, info, false);
}

// ------------------------------------------------------------------------------------------------ include/fluca_hip_implicit_ranks.h

extern "C" int fl_scalar_diffusion_apply_ranks(fl_scalar *m, double c, const double *phi_dev, double *out_dev) { return diffusion_apply(m, c, phi_dev, out_dev, true); }

extern "C" int fl_scalar_diffusion_solve_ranks(fl_scalar *m, double c, double rtol, int maxit, const double *b_dev, double *x_dev, fl_scalar_cheb_info *info)
{
  return diffusion_solve(m, c, rtol, maxit, b_dev, x_dev, info, true);
}

extern "C" int fl_scalar_step_imex_ranks(fl_scalar *m, double dt, int nstages, double theta, double rtol, int maxit, const double *source_dev, double *phi_dev,
                                         fl_scalar_cheb_info *info)
{
  return step_imex(m, dt, nstages, theta, rtol, maxit, source_dev, phi_dev, info, true);
}
