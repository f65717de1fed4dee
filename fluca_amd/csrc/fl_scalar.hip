// fl_scalar.hip -- transport of a passive scalar phi (cell centres) by the face velocities V: the right-hand side
//     R(phi)(c) = - sum_d [ V_d(f+) phi_f(f+) - V_d(f-) phi_f(f-) ] / h_d(c) + Gamma sum_d [ g_d(f+) - g_d(f-) ] / h_d(c) + q(c)
// with the limited second-order TVD face value phi_f of FlucaFDSecondOrderTVD (fluca/src/fd/impls/secondordertvd/secondordertvd.c:187-356), the
// two-point face gradient g, and one stage of the s-stage second-order SSP Runge-Kutta method of the reference's tutorials (-ts_type ssp, rks2)
// fused into the same sweep:  out = c0 phi^n + c1 w + c2 R(w).  DESIGN.md section 4 has the boundary rules and where they leave the reference.
//
// 13-point window, two cells to either side along every axis; nonlinear (upwind side from the sign of V, a limiter of a gradient ratio), so there
// are no rows to pre-multiply: a cell forms its six face values from the five cells of w along each axis.  w 8 + V 24 + out 8 = 40 B/cell of
// compulsory traffic (48 in the stage that also reads phi^n).  The sweep is k_schur_var's (fl_schur_var.hip): no LDS, a lane owns one cell of
// a 64-cell row segment, the rows dealt so that an XCD works through one band of y plane after plane.  What differs: w is read from the caller's
// UNPADDED array -- a cell outside the line is its periodic image (fetched from where it lives) or is replaced by the boundary rule, so no
// copy into a padded vector and no ghost fill stand between two stages, and a stage is one launch.  One rank only (fl_scalar_create).
#include "fl_device.h"
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

// phi_f = phi_u + alpha psi(r) (phi_d - phi_u), r = g_u / g_c guarded as in the reference
template <int L>
__device__ __forceinline__ double sc_face(bool up, double Pm, double Pp, double Gm, double Gc, double Gp, double ap, double am)
{
  const double pu = up ? Pm : Pp, pd = up ? Pp : Pm, gu = up ? Gm : Gp, al = up ? ap : am;
  const double r = fabs(Gc) > 1e-30 ? gu / Gc : 1.;
  return pu + al * limiter<L>(r) * (pd - pu);
}

// The contribution of one axis to R at cell a of a line: [ -(V1 f1 - V0 f0) + Gamma (g(a+1) - g(a)) ] / h_a, with V0 / V1 the velocities
// of the faces a / a+1.  klo / khi, vlo / vhi: kind and value of the boundaries at the ends of the axis (unused where it wraps).
template <int L>
__device__ __forceinline__ double sc_axis(const ScCell &T, const double *__restrict__ w, int a, int n, bool wraps, int klo, int khi, double vlo, double vhi, double dlo, double dhi,
                                          int64_t c0, int64_t cs, double V0, double V1, double gamma)
{
  double       P0 = sc_ld(w, c0, cs, a - 2, n, wraps), P1 = sc_ld(w, c0, cs, a - 1, n, wraps), P3 = sc_ld(w, c0, cs, a + 1, n, wraps), P4 = sc_ld(w, c0, cs, a + 2, n, wraps);
  const double P2 = w[c0 + a * cs];
  const bool   lo0 = !wraps && a == 0, lo1 = !wraps && a == 1, hi0 = !wraps && a == n - 1, hi1 = !wraps && a == n - 2;
  // Dirichlet: the boundary value stands where the cell beyond the boundary would (the table's 1 / distance is that of centre -- face)
  if (klo == 0) {
    if (lo0) P1 = vlo;
    if (lo1) P0 = vlo;
  }
  if (khi == 0) {
    if (hi0) P3 = vhi;
    if (hi1) P4 = vhi;
  }
  double G0 = (P1 - P0) * T.ic0, G1 = (P2 - P1) * T.ic1, G2 = (P3 - P2) * T.ic2, G3 = (P4 - P3) * T.ic3;  // the gradients of the faces a-1 .. a+2
  // Neumann: the gradient of the boundary face is the value itself
  if (klo == 1) {
    if (lo0) G1 = vlo;
    if (lo1) G0 = vlo;
  }
  if (khi == 1) {
    if (hi0) G2 = vhi;
    if (hi1) G3 = vhi;
  }
  double f0 = sc_face<L>(V0 > 0., P1, P2, G0, G1, G2, T.ap0, T.am0), f1 = sc_face<L>(V1 > 0., P2, P3, G1, G2, G3, T.ap1, T.am1);
  // a boundary face carries the boundary's own value for either flow direction
  if (lo0) f0 = klo == 0 ? vlo : P2 - dlo * vlo;
  if (hi0) f1 = khi == 0 ? vhi : P2 + dhi * vhi;
  return (gamma * (G2 - G1) - (V1 * f1 - V0 * f0)) * T.ih;
}

// out = c0 phin + c1 w + c2 (R(w) + q).  HASN = false: phin is not read (c0 is not used).  phin may be out (the last stage of a step in place: a
// cell's phin is read by the lane that writes it); out is never w.  Grid: a multiple of 8 blocks; block b works for XCD b % 8 on the y band of it.
// Blocks per CU: four (128 registers a lane) hold every limiter but venkatakrishnan, whose two rational functions need 131: three there, not scratch.
constexpr int sc_minblocks(int L) { return L == LIM_VENKATAKRISHNAN ? 3 : 4; }
template <int L, bool HASN>
__global__ void __launch_bounds__(256, sc_minblocks(L)) k_scalar_stage(ScGrid g, double c0, double c1, double c2, const double *phin, const double *__restrict__ w,
                                                                     const double *__restrict__ Vx, const double *__restrict__ Vy, const double *__restrict__ Vz,
                                                                     const double *__restrict__ q, double *out)
{
  const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), nw = blockDim.x >> 6;
  const int xcd = blockIdx.x & 7, lb = blockIdx.x >> 3, nlb = gridDim.x >> 3;
  const int band = (g.ny + 7) / 8, j0 = xcd * band, j1 = min(j0 + band, g.ny);
  if (j0 >= j1) return;
  const int     nseg = (g.nx + 63) / 64, nj = j1 - j0;
  const int64_t nitem = (int64_t)nseg * nj * g.nz, nxy = (int64_t)g.nx * g.ny;
  const bool    wx = g.per & 1, wy = g.per & 2, wz = g.per & 4;
  const int     fx = wx ? g.nx : g.nx + 1, fy = wy ? g.ny : g.ny + 1;
  // (as in k_schur_var) a wave keeps ONE x segment for all its rows whenever the launch allows it: the x rows of its cells are fetched once
  const bool   fixed_seg = ((int64_t)nlb * nw) % nseg == 0;
  const int    seg0 = (int)(((int64_t)lb * nw + wv) % nseg), i0 = min(seg0 * 64 + lane, g.nx - 1);
  const ScCell X0 = g.c[0][i0];
  for (int64_t it = (int64_t)lb * nw + wv; it < nitem; it += (int64_t)nlb * nw) {
    const int seg = (int)(it % nseg), row = (int)(it / nseg);
    const int j = j0 + row % nj, k = row / nj, i = seg * 64 + lane;
    if (i >= g.nx) continue;
    const int64_t urow = ((int64_t)k * g.ny + j) * g.nx, c = urow + i;
    const int     ip = (i + 1 == g.nx && wx) ? 0 : i + 1, jp = (j + 1 == g.ny && wy) ? 0 : j + 1, kp = (k + 1 == g.nz && wz) ? 0 : k + 1;
    const int64_t vxr = ((int64_t)k * g.ny + j) * fx, vyr = (int64_t)k * fy * g.nx + i;
    double acc = sc_axis<L>(fixed_seg ? X0 : g.c[0][i], w, i, g.nx, wx, g.kind[0], g.kind[1], g.val[0], g.val[1], g.dlo[0], g.dhi[0], urow, 1, Vx[vxr + i], Vx[vxr + ip], g.gamma);
    acc += sc_axis<L>(g.c[1][j], w, j, g.ny, wy, g.kind[2], g.kind[3], g.val[2], g.val[3], g.dlo[1], g.dhi[1], (int64_t)k * nxy + i, g.nx, Vy[vyr + (int64_t)j * g.nx],
                      Vy[vyr + (int64_t)jp * g.nx], g.gamma);
    acc += sc_axis<L>(g.c[2][k], w, k, g.nz, wz, g.kind[4], g.kind[5], g.val[4], g.val[5], g.dlo[2], g.dhi[2], (int64_t)j * g.nx + i, nxy, Vz[c], Vz[(int64_t)kp * nxy + (int64_t)j * g.nx + i],
                      g.gamma);
    if (q) acc += __builtin_nontemporal_load(q + c);
    double r = c1 * w[c] + c2 * acc;
    if (HASN) r += c0 * __builtin_nontemporal_load(phin + c);
    __builtin_nontemporal_store(r, out + c);
  }
}

// ---- reductions over the cells: per-block partial results, finished on the host in block order (the same bits on every call)
__device__ __forceinline__ void sc_block3(double &mn, double &mx, double &sm, double *red, double *out)
{
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    mn = fmin(mn, __shfl_down(mn, o, 64));
    mx = fmax(mx, __shfl_down(mx, o, 64));
    sm += __shfl_down(sm, o, 64);
  }
  if (lane == 0) {
    red[wv]     = mn;
    red[4 + wv] = mx;
    red[8 + wv] = sm;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    out[3 * blockIdx.x]     = fmin(fmin(red[0], red[1]), fmin(red[2], red[3]));
    out[3 * blockIdx.x + 1] = fmax(fmax(red[4], red[5]), fmax(red[6], red[7]));
    out[3 * blockIdx.x + 2] = (red[8] + red[9]) + (red[10] + red[11]);
  }
}

// partial[3 b ..]: min phi, max phi, sum phi vol over the cells of block b; hx / hy / hz: the face-to-face widths
__global__ void __launch_bounds__(256) k_scalar_stats(int nx, int ny, int nz, const double *__restrict__ hx, const double *__restrict__ hy, const double *__restrict__ hz,
                                                      const double *__restrict__ phi, double *__restrict__ partial)
{
  __shared__ double red[12];
  const int64_t     N  = (int64_t)nx * ny * nz;
  double            mn = INFINITY, mx = -INFINITY, sm = 0.;
  for (int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x; c < N; c += (int64_t)gridDim.x * 256) {
    const int     i = (int)(c % nx);
    const int64_t t = c / nx;
    const double  v = phi[c];
    mn = fmin(mn, v);
    mx = fmax(mx, v);
    sm += v * (hx[i] * hy[t % ny] * hz[t / ny]);
  }
  sc_block3(mn, mx, sm, red, partial);
}

// partial[3 b ..]: -, max dt sum_d max(|V(f-)|, |V(f+)|) / h_d, max Gamma dt sum_d 2 / h_d^2 (kept in the slots of the maximum and -- as a maximum
// of non-negative numbers against 0 -- of the sum's)
__global__ void __launch_bounds__(256) k_scalar_cfl(int nx, int ny, int nz, int per, double dt, double gamma, const double *__restrict__ hx, const double *__restrict__ hy,
                                                    const double *__restrict__ hz, const double *__restrict__ Vx, const double *__restrict__ Vy, const double *__restrict__ Vz,
                                                    double *__restrict__ partial)
{
  __shared__ double red[12];
  const int64_t     N = (int64_t)nx * ny * nz, nxy = (int64_t)nx * ny;
  const bool        wx = per & 1, wy = per & 2, wz = per & 4;
  const int         fx = wx ? nx : nx + 1, fy = wy ? ny : ny + 1;
  double            mn = 0., ca = 0., cd = 0.;
  for (int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x; c < N; c += (int64_t)gridDim.x * 256) {
    const int     i = (int)(c % nx);
    const int64_t t = c / nx;
    const int     j = (int)(t % ny), k = (int)(t / ny);
    const int     ip = (i + 1 == nx && wx) ? 0 : i + 1, jp = (j + 1 == ny && wy) ? 0 : j + 1, kp = (k + 1 == nz && wz) ? 0 : k + 1;
    const int64_t vxr = ((int64_t)k * ny + j) * fx, vyr = (int64_t)k * fy * nx + i;
    const double  ax = fmax(fabs(Vx[vxr + i]), fabs(Vx[vxr + ip])), ay = fmax(fabs(Vy[vyr + (int64_t)j * nx]), fabs(Vy[vyr + (int64_t)jp * nx])),
                 az = fmax(fabs(Vz[c]), fabs(Vz[(int64_t)kp * nxy + (int64_t)j * nx + i]));
    const double a = hx[i], b = hy[j], d = hz[k];
    ca = fmax(ca, dt * (ax / a + ay / b + az / d));
    cd = fmax(cd, gamma * dt * (2. / (a * a) + 2. / (b * b) + 2. / (d * d)));
  }
  // (both are maxima: the sum's slot is reduced by hand below)
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    ca = fmax(ca, __shfl_down(ca, o, 64));
    cd = fmax(cd, __shfl_down(cd, o, 64));
  }
  if (lane == 0) {
    red[wv]     = ca;
    red[4 + wv] = cd;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    partial[3 * blockIdx.x]     = mn;
    partial[3 * blockIdx.x + 1] = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
    partial[3 * blockIdx.x + 2] = fmax(fmax(red[4], red[5]), fmax(red[6], red[7]));
  }
}

}  // namespace fl

using namespace fl;

// ------------------------------------------------------------------------------------------------ limiters on the host

namespace {

const char *const LIMITER_NAMES[LIM_COUNT] = {"superbee", "minmod", "mc", "vanleer", "vanalbada", "barthjesperson", "venkatakrishnan", "koren", "upwind", "sou", "quick"};

template <int L>
double limiter_host(double r) { return limiter<L>(r); }
typedef double (*LimiterFn)(double);
const LimiterFn LIMITER_HOST[LIM_COUNT] = {limiter_host<0>, limiter_host<1>, limiter_host<2>, limiter_host<3>, limiter_host<4>, limiter_host<5>,
                                           limiter_host<6>, limiter_host<7>, limiter_host<8>, limiter_host<9>, limiter_host<10>};

}  // namespace

extern "C" int fl_limiter_from_name(const char *name, int *limiter)
{
  if (!name || !limiter) return FL_ERR_ARG_NULL;
  for (int l = 0; l < LIM_COUNT; ++l)
    if (!std::strcmp(name, LIMITER_NAMES[l])) {
      *limiter = l;
      return FL_SUCCESS;
    }
  return FL_ERR_ARG_OUTOFRANGE;
}

extern "C" int fl_limiter_eval(int limiter, double r, double *psi)
{
  if (!psi) return FL_ERR_ARG_NULL;
  if (limiter < 0 || limiter >= LIM_COUNT) return FL_ERR_ARG_OUTOFRANGE;
  *psi = LIMITER_HOST[limiter](r);
  return FL_SUCCESS;
}

// ------------------------------------------------------------------------------------------------ the handle

struct fl_scalar {
  fl_poisson   *h = nullptr;  // borrowed: grid, device, stream
  ScGrid        g;
  int           limiter = LIM_SUPERBEE;
  const double *V[3] = {nullptr, nullptr, nullptr};  // borrowed
  void         *tab[3] = {nullptr, nullptr, nullptr};
  double       *hw[3] = {nullptr, nullptr, nullptr};  // face-to-face widths
  double       *work[2] = {nullptr, nullptr};         // the two stage vectors of fl_scalar_step
  double       *partial = nullptr;                    // 3 * SC_REDUCE_BLOCKS
  std::vector<double> partial_host;
};

constexpr int SC_REDUCE_BLOCKS = 1024;

// The launch of k_scalar_stage: the XCD band plan of k_schur_var with this kernel's residency (sc_minblocks blocks on each of an XCD's 32 CUs).
// Host arithmetic only.
struct ScalarPlan {
  int     per_xcd, nseg, band, fixed_seg;
  int64_t items;
};
static ScalarPlan scalar_plan(int nx, int ny, int nz, int limiter)
{
  ScalarPlan pl;
  pl.nseg      = (nx + 63) / 64;
  pl.band      = (ny + 7) / 8;
  pl.items     = (int64_t)pl.nseg * ny * nz;
  pl.per_xcd   = (int)std::max<int64_t>(1, std::min<int64_t>((pl.items / 8 + 3) / 4, 32 * sc_minblocks(limiter)));  // every block resident, no block without a row segment
  pl.fixed_seg = ((int64_t)pl.per_xcd * 4) % pl.nseg == 0 ? 1 : 0;                                         // the kernel's own test, with its four waves per block
  return pl;
}

// Not part of the public C-ABI (tests): the plan of k_scalar_stage<limiter> on an nx x ny x nz block -- 0 per_xcd, 1 nseg, 2 band, 3 fixed_seg, 4 items.
// A query of its own rather than fields of fldbg_launch_plans, whose count its callers check.
extern "C" int fldbg_scalar_plan(int nx, int ny, int nz, int limiter, int *out, int nout)
{
  if (nx < 1 || ny < 1 || nz < 1 || limiter < 0 || limiter >= LIM_COUNT) return FL_ERR_ARG_OUTOFRANGE;
  if (!out) return 5;
  if (nout < 5) return FL_ERR_ARG_SIZ;
  const ScalarPlan pl = scalar_plan(nx, ny, nz, limiter);
  if (pl.items > INT32_MAX) return FL_ERR_ARG_OUTOFRANGE;
  out[0] = pl.per_xcd; out[1] = pl.nseg; out[2] = pl.band; out[3] = pl.fixed_seg; out[4] = (int)pl.items;
  return 5;
}

namespace {

struct StageArgs {
  double        c0, c1, c2;
  const double *phin, *w, *q;
  double       *out;
};

template <int L>
void launch_stage(const fl_scalar *m, const StageArgs &a)
{
  const dim3 grid(8 * scalar_plan(m->g.nx, m->g.ny, m->g.nz, L).per_xcd);
  if (a.phin) hipLaunchKernelGGL((k_scalar_stage<L, true>), grid, dim3(256), 0, m->h->stream, m->g, a.c0, a.c1, a.c2, a.phin, a.w, m->V[0], m->V[1], m->V[2], a.q, a.out);
  else hipLaunchKernelGGL((k_scalar_stage<L, false>), grid, dim3(256), 0, m->h->stream, m->g, a.c0, a.c1, a.c2, a.phin, a.w, m->V[0], m->V[1], m->V[2], a.q, a.out);
}
typedef void (*StageFn)(const fl_scalar *, const StageArgs &);
// the limiter is a template parameter: eleven kernels, none of which branches on it (profiles/scalar_devcode.txt)
const StageFn STAGE[LIM_COUNT] = {launch_stage<0>, launch_stage<1>, launch_stage<2>, launch_stage<3>, launch_stage<4>, launch_stage<5>,
                                  launch_stage<6>, launch_stage<7>, launch_stage<8>, launch_stage<9>, launch_stage<10>};

int scalar_init(fl_scalar *m, fl_poisson *h, const int bc[6])
{
  m->h = h;
  FL_HIP(hipSetDevice(h->device));
  ScGrid &g = m->g;
  std::memset(&g, 0, sizeof(g));
  g.nx = h->g.nx; g.ny = h->g.ny; g.nz = h->g.nz;
  for (int d = 0; d < 3; ++d) {
    const Axis &A = h->ax[d];
    g.per |= A.periodic ? 1 << d : 0;
    g.kind[2 * d] = bc[2 * d];
    g.kind[2 * d + 1] = bc[2 * d + 1];
    g.dlo[d] = A.xcc(0) - A.xf[0];
    g.dhi[d] = A.xf[(size_t)A.n] - A.xcc(A.n - 1);
    std::vector<ScCell> rows;
    FL_CHK(build_axis_scalar(A, rows));
    std::vector<double> hw((size_t)A.n);
    for (int64_t i = 0; i < A.n; ++i) hw[(size_t)i] = A.xf[(size_t)i + 1] - A.xf[(size_t)i];
    FL_HIP(hipMalloc(&m->tab[d], sizeof(ScCell) * rows.size()));
    FL_HIP(hipMalloc((void **)&m->hw[d], sizeof(double) * hw.size()));
    FL_HIP(hipMemcpy(m->tab[d], rows.data(), sizeof(ScCell) * rows.size(), hipMemcpyHostToDevice));
    FL_HIP(hipMemcpy(m->hw[d], hw.data(), sizeof(double) * hw.size(), hipMemcpyHostToDevice));
    g.c[d] = (const ScCell *)m->tab[d];
  }
  FL_HIP(hipMalloc((void **)&m->partial, sizeof(double) * 3 * SC_REDUCE_BLOCKS));
  m->partial_host.resize((size_t)3 * SC_REDUCE_BLOCKS);
  return FL_SUCCESS;
}

int reduce_blocks(const fl_scalar *m) { return (int)std::max<int64_t>(1, std::min<int64_t>((m->h->ncell + 255) / 256, SC_REDUCE_BLOCKS)); }

int fetch_partials(fl_scalar *m, int nb)
{
  FL_HIP(hipGetLastError());
  FL_HIP(hipMemcpyAsync(m->partial_host.data(), m->partial, sizeof(double) * 3 * (size_t)nb, hipMemcpyDeviceToHost, m->h->stream));
  FL_HIP(hipStreamSynchronize(m->h->stream));
  return FL_SUCCESS;
}

}  // namespace

extern "C" int fl_scalar_destroy(fl_scalar *m)
{
  if (!m) return FL_SUCCESS;
  if (m->h) {
    (void)hipSetDevice(m->h->device);
    if (m->h->stream) (void)hipStreamSynchronize(m->h->stream);
  }
  for (int d = 0; d < 3; ++d) {
    if (m->tab[d]) (void)hipFree(m->tab[d]);
    if (m->hw[d]) (void)hipFree(m->hw[d]);
  }
  for (double *p : {m->work[0], m->work[1], m->partial})
    if (p) (void)hipFree(p);
  delete m;
  return FL_SUCCESS;
}

extern "C" int fl_scalar_create(fl_poisson *grid_from, const int bc[6], fl_scalar **out)
{
  if (!grid_from || !bc || !out) return FL_ERR_ARG_NULL;
  *out = nullptr;
  for (int b = 0; b < 6; ++b)
    if (bc[b] < 0 || bc[b] > 2) return FL_ERR_ARG_OUTOFRANGE;
  for (int d = 0; d < 3; ++d)
    if ((bc[2 * d] == 2) != grid_from->ax[d].periodic || (bc[2 * d + 1] == 2) != grid_from->ax[d].periodic) return FL_ERR_ARG_WRONG;
  if (grid_from->multi) return FL_ERR_SUP;  // several ranks: a two-deep ghost of phi and a ring of V (as k_schur_var_ring has) are not built
  fl_scalar *m  = new fl_scalar();
  const int  rc = scalar_init(m, grid_from, bc);
  if (rc) {
    fl_scalar_destroy(m);
    return rc;
  }
  *out = m;
  return FL_SUCCESS;
}

extern "C" int fl_scalar_set_boundary_value(fl_scalar *m, int boundary, double value)
{
  if (!m) return FL_ERR_ARG_NULL;
  if (boundary < 0 || boundary > 5 || !std::isfinite(value)) return FL_ERR_ARG_OUTOFRANGE;
  m->g.val[boundary] = value;
  return FL_SUCCESS;
}

extern "C" int fl_scalar_set_limiter(fl_scalar *m, int limiter)
{
  if (!m) return FL_ERR_ARG_NULL;
  if (limiter < 0 || limiter >= LIM_COUNT) return FL_ERR_ARG_OUTOFRANGE;
  m->limiter = limiter;
  return FL_SUCCESS;
}

extern "C" int fl_scalar_set_diffusivity(fl_scalar *m, double gamma)
{
  if (!m) return FL_ERR_ARG_NULL;
  if (!(gamma >= 0.) || !std::isfinite(gamma)) return FL_ERR_ARG_OUTOFRANGE;
  m->g.gamma = gamma;
  return FL_SUCCESS;
}

extern "C" int fl_scalar_set_velocity(fl_scalar *m, const double *Vx_dev, const double *Vy_dev, const double *Vz_dev)
{
  if (!m || !Vx_dev || !Vy_dev || !Vz_dev) return FL_ERR_ARG_NULL;
  m->V[0] = Vx_dev;
  m->V[1] = Vy_dev;
  m->V[2] = Vz_dev;
  return FL_SUCCESS;
}

extern "C" int fl_scalar_rhs(fl_scalar *m, const double *phi_dev, const double *source_dev, double *out_dev)
{
  if (!m || !phi_dev || !out_dev) return FL_ERR_ARG_NULL;
  if (phi_dev == out_dev) return FL_ERR_ARG_WRONG;  // neighbours still read phi
  if (!m->V[0]) return FL_ERR_ARG_WRONGSTATE;
  FL_HIP(hipSetDevice(m->h->device));
  STAGE[m->limiter](m, StageArgs{0., 0., 1., nullptr, phi_dev, source_dev, out_dev});
  FL_HIP(hipGetLastError());
  return FL_SUCCESS;
}

// w <- phi; s - 1 times w <- w + dt / (s - 1) R(w); phi <- ((s - 1) w + phi + dt R(w)) / s.  One launch per stage; the stage vectors alternate between
// the handle's two work arrays, and the last stage writes phi in place (it reads of phi only the cell it writes).
extern "C" int fl_scalar_step(fl_scalar *m, double dt, int nstages, const double *source_dev, double *phi_dev)
{
  if (!m || !phi_dev) return FL_ERR_ARG_NULL;
  if (nstages < 2 || !std::isfinite(dt)) return FL_ERR_ARG_OUTOFRANGE;
  if (!m->V[0]) return FL_ERR_ARG_WRONGSTATE;
  FL_HIP(hipSetDevice(m->h->device));
  for (int a = 0; a < (nstages > 2 ? 2 : 1); ++a)
    if (!m->work[a]) FL_HIP(hipMalloc((void **)&m->work[a], sizeof(double) * (size_t)m->h->ncell));
  const int     s = nstages;
  const double *w = phi_dev;
  for (int st = 0; st < s - 1; ++st) {
    double *o = m->work[st & 1];
    STAGE[m->limiter](m, StageArgs{0., 1., dt / (s - 1), nullptr, w, source_dev, o});
    w = o;
  }
  STAGE[m->limiter](m, StageArgs{1. / s, (s - 1.) / s, dt / s, phi_dev, w, source_dev, phi_dev});
  FL_HIP(hipGetLastError());
  return FL_SUCCESS;
}

extern "C" int fl_scalar_cfl(fl_scalar *m, double dt, double out[2])
{
  if (!m || !out) return FL_ERR_ARG_NULL;
  if (!m->V[0]) return FL_ERR_ARG_WRONGSTATE;
  FL_HIP(hipSetDevice(m->h->device));
  const int nb = reduce_blocks(m);
  hipLaunchKernelGGL(k_scalar_cfl, dim3(nb), dim3(256), 0, m->h->stream, m->g.nx, m->g.ny, m->g.nz, m->g.per, dt, m->g.gamma, m->hw[0], m->hw[1], m->hw[2], m->V[0], m->V[1], m->V[2],
                     m->partial);
  FL_CHK(fetch_partials(m, nb));
  out[0] = out[1] = 0.;
  for (int b = 0; b < nb; ++b) {
    out[0] = std::max(out[0], m->partial_host[(size_t)3 * b + 1]);
    out[1] = std::max(out[1], m->partial_host[(size_t)3 * b + 2]);
  }
  return FL_SUCCESS;
}

extern "C" int fl_scalar_stats(fl_scalar *m, const double *phi_dev, double out[3])
{
  if (!m || !phi_dev || !out) return FL_ERR_ARG_NULL;
  FL_HIP(hipSetDevice(m->h->device));
  const int nb = reduce_blocks(m);
  hipLaunchKernelGGL(k_scalar_stats, dim3(nb), dim3(256), 0, m->h->stream, m->g.nx, m->g.ny, m->g.nz, m->hw[0], m->hw[1], m->hw[2], phi_dev, m->partial);
  FL_CHK(fetch_partials(m, nb));
  out[0] = m->partial_host[0];
  out[1] = m->partial_host[1];
  out[2] = 0.;
  for (int b = 0; b < nb; ++b) {
    out[0] = std::min(out[0], m->partial_host[(size_t)3 * b]);
    out[1] = std::max(out[1], m->partial_host[(size_t)3 * b + 1]);
    out[2] += m->partial_host[(size_t)3 * b + 2];
  }
  return FL_SUCCESS;
}
