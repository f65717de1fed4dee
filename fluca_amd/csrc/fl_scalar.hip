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
// copy into a padded vector and no ghost fill stand between two stages, and a stage is one launch.
//
// Several ranks (fl_scalar_create_ranks, k_scalar_stage_ring): the same sweep over the rank's block.  Behind an end of an axis where a neighbouring
// rank sits, the cells -2, -1 / n, n+1 of w come from a GHOST SLAB -- two planes of the neighbour's outermost cells, [layer][line in the plane],
// the plane's fast index the block's fastest in-plane axis (the y and z slabs are read x-contiguously by a wave) -- and the boundary rule does not
// apply: the cell is an interior cell.  The window is a star, so no edge or corner cells travel: at most six slabs, one exchange per stage.  The
// velocity of the face n the next rank owns is the handle's hiface plane (fl_fill_hifaces).  A stage that is not the last of a step stores the cells
// it writes within two layers of a rank face into that boundary's send slab as well, so one exchange and one launch stand between two stages.
// The exchange is NOT overlapped with the sweep: that would take a second launch over a shell that is a few per cent of the block (as k_schur_var_ring).
#include "fl_device.h"
#include "fl_handle.h"
#include "fl_limiter.h"
#include "fl_scalar_handle.h"

namespace fl {

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
// RING (k_scalar_stage_ring): the five cells may come from the slabs of e, and an end with a neighbouring rank is no physical boundary -- the cell
// behind it is an interior cell.  Only the five loads and the predicates lo0 / lo1 / hi0 / hi1 differ; the arithmetic is this one piece of source.
template <int L, bool RING>
__device__ __forceinline__ double sc_axis(const ScCell &T, const double *__restrict__ w, int a, int n, bool wraps, int klo, int khi, double vlo, double vhi, double dlo, double dhi,
                                          int64_t c0, int64_t cs, double V0, double V1, double gamma, const ScEnds &e)
{
  double P0, P1, P3, P4;
  bool   lo0, lo1, hi0, hi1;
  if constexpr (RING) {
    P0 = sc_ld_ring(w, c0, cs, a - 2, n, wraps, e), P1 = sc_ld_ring(w, c0, cs, a - 1, n, wraps, e), P3 = sc_ld_ring(w, c0, cs, a + 1, n, wraps, e), P4 = sc_ld_ring(w, c0, cs, a + 2, n, wraps, e);
  } else {
    P0 = sc_ld(w, c0, cs, a - 2, n, wraps), P1 = sc_ld(w, c0, cs, a - 1, n, wraps), P3 = sc_ld(w, c0, cs, a + 1, n, wraps), P4 = sc_ld(w, c0, cs, a + 2, n, wraps);
  }
  const double P2 = w[c0 + a * cs];
  if constexpr (RING) {
    const bool plo = !wraps && !e.nlo, phi = !wraps && !e.nhi;
    lo0 = plo && a == 0, lo1 = plo && a == 1, hi0 = phi && a == n - 1, hi1 = phi && a == n - 2;
  } else {
    lo0 = !wraps && a == 0, lo1 = !wraps && a == 1, hi0 = !wraps && a == n - 1, hi1 = !wraps && a == n - 2;
  }
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
  const ScEnds none = {false, false, nullptr, 0, 0};  // (one rank: not read)
  for (int64_t it = (int64_t)lb * nw + wv; it < nitem; it += (int64_t)nlb * nw) {
    const int seg = (int)(it % nseg), row = (int)(it / nseg);
    const int j = j0 + row % nj, k = row / nj, i = seg * 64 + lane;
    if (i >= g.nx) continue;
    const int64_t urow = ((int64_t)k * g.ny + j) * g.nx, c = urow + i;
    const int     ip = (i + 1 == g.nx && wx) ? 0 : i + 1, jp = (j + 1 == g.ny && wy) ? 0 : j + 1, kp = (k + 1 == g.nz && wz) ? 0 : k + 1;
    const int64_t vxr = ((int64_t)k * g.ny + j) * fx, vyr = (int64_t)k * fy * g.nx + i;
    double acc = sc_axis<L, false>(fixed_seg ? X0 : g.c[0][i], w, i, g.nx, wx, g.kind[0], g.kind[1], g.val[0], g.val[1], g.dlo[0], g.dhi[0], urow, 1, Vx[vxr + i], Vx[vxr + ip], g.gamma, none);
    acc += sc_axis<L, false>(g.c[1][j], w, j, g.ny, wy, g.kind[2], g.kind[3], g.val[2], g.val[3], g.dlo[1], g.dhi[1], (int64_t)k * nxy + i, g.nx, Vy[vyr + (int64_t)j * g.nx],
                      Vy[vyr + (int64_t)jp * g.nx], g.gamma, none);
    acc += sc_axis<L, false>(g.c[2][k], w, k, g.nz, wz, g.kind[4], g.kind[5], g.val[4], g.val[5], g.dlo[2], g.dhi[2], (int64_t)j * g.nx + i, nxy, Vz[c], Vz[(int64_t)kp * nxy + (int64_t)j * g.nx + i],
                      g.gamma, none);
    if (q) acc += __builtin_nontemporal_load(q + c);
    double r = c1 * w[c] + c2 * acc;
    if (HASN) r += c0 * __builtin_nontemporal_load(phin + c);
    __builtin_nontemporal_store(r, out + c);
  }
}

// What a rank's block of several reads and writes beside its own arrays (all wave-uniform: scalar registers).  recv / send: the slabs received and
// sent, ONE array each -- 31 separate pointers and flags cost the kernel scalar registers it does not have -- of four layers per axis, the axes one
// after the other: layers 0, 1 of axis d belong to its low end, 2, 3 to its high end (so a cell m outside the line is layer m + 2 or m - n + 2 of
// recv, and the cells 0, 1 / n-2, n-1 are the layers 0, 1 / 2, 3 of send).  vhi[d]: the velocity of the face n of axis d where the next rank owns it (the
// handle's hiface plane).  pack: the boundaries (bits as nb) whose send layers this stage fills -- 0 in the last stage of a step and in fl_scalar_rhs.
struct ScRing {
  const double *recv, *vhi[3];
  double       *send;
  int           pack;
};

// k_scalar_stage on one rank's block of several; nb: bit 2 d / 2 d + 1 = a neighbouring rank behind the low / high end of axis d.  g: the block (per: the
// periodic axes the rank holds alone), the tables cut to its rows.  A cell within two layers of a rank face is also stored into that face's send
// layers (what the peer reads as its cells n, n+1 / -2, -1).
template <int L, bool HASN>
__global__ void __launch_bounds__(256, sc_minblocks(L)) k_scalar_stage_ring(ScGrid g, ScRing rg, int nb, double c0, double c1, double c2, const double *phin, const double *__restrict__ w,
                                                                          const double *__restrict__ Vx, const double *__restrict__ Vy, const double *__restrict__ Vz,
                                                                          const double *__restrict__ q, double *out)
{
  const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), nw = blockDim.x >> 6;
  const int xcd = blockIdx.x & 7, lb = blockIdx.x >> 3, nlb = gridDim.x >> 3;
  const int band = (g.ny + 7) / 8, j0 = xcd * band, j1 = min(j0 + band, g.ny);
  if (j0 >= j1) return;
  const int     nseg = (g.nx + 63) / 64, nj = j1 - j0;
  const int64_t nitem = (int64_t)nseg * nj * g.nz, nxy = (int64_t)g.nx * g.ny, nyz = (int64_t)g.ny * g.nz, nxz = (int64_t)g.nx * g.nz;
  const bool    wx = g.per & 1, wy = g.per & 2, wz = g.per & 4;
  const bool    lx = nb & 1, hx = nb & 2, ly = nb & 4, hy = nb & 8, lz = nb & 16, hz = nb & 32;
  const int     fx = (wx || hx) ? g.nx : g.nx + 1, fy = (wy || hy) ? g.ny : g.ny + 1;  // the faces the block owns along x / y
  const bool    fixed_seg = ((int64_t)nlb * nw) % nseg == 0;
  const int     seg0 = (int)(((int64_t)lb * nw + wv) % nseg), i0 = min(seg0 * 64 + lane, g.nx - 1);
  const ScCell  X0 = g.c[0][i0];
  for (int64_t it = (int64_t)lb * nw + wv; it < nitem; it += (int64_t)nlb * nw) {
    const int seg = (int)(it % nseg), row = (int)(it / nseg);
    const int j = j0 + row % nj, k = row / nj, i = seg * 64 + lane;
    if (i >= g.nx) continue;
    const int64_t urow = ((int64_t)k * g.ny + j) * g.nx, c = urow + i;
    const int64_t prx = (int64_t)k * g.ny + j, pry = (int64_t)k * g.nx + i, prz = (int64_t)j * g.nx + i;  // this cell's line in the planes across x / y / z
    const int     ip = (i + 1 == g.nx && wx) ? 0 : i + 1, jp = (j + 1 == g.ny && wy) ? 0 : j + 1, kp = (k + 1 == g.nz && wz) ? 0 : k + 1;
    const int64_t vxr = prx * fx, vyr = (int64_t)k * fy * g.nx + i;
    // the face behind the last cell where the next rank owns it: the hiface plane
    const double *v1x = (hx && i + 1 == g.nx) ? rg.vhi[0] + prx : Vx + vxr + ip, *v1y = (hy && j + 1 == g.ny) ? rg.vhi[1] + pry : Vy + vyr + (int64_t)jp * g.nx,
                 *v1z = (hz && k + 1 == g.nz) ? rg.vhi[2] + prz : Vz + (int64_t)kp * nxy + prz;
    // (of the x row a wave with a fixed segment keeps the first six numbers; ap1, am1 and ih -- two 16-byte loads -- are fetched with every row: kept
    // as well, they are the registers that the slab reads and the pack need, and one of them went to scratch)
    ScCell TX = g.c[0][i];
    if (fixed_seg) { TX.ic0 = X0.ic0; TX.ic1 = X0.ic1; TX.ic2 = X0.ic2; TX.ic3 = X0.ic3; TX.ap0 = X0.ap0; TX.am0 = X0.am0; }
    double acc = sc_axis<L, true>(TX, w, i, g.nx, wx, g.kind[0], g.kind[1], g.val[0], g.val[1], g.dlo[0], g.dhi[0], urow, 1, Vx[vxr + i], *v1x, g.gamma,
                                  ScEnds{lx, hx, rg.recv, nyz, prx});
    acc += sc_axis<L, true>(g.c[1][j], w, j, g.ny, wy, g.kind[2], g.kind[3], g.val[2], g.val[3], g.dlo[1], g.dhi[1], (int64_t)k * nxy + i, g.nx, Vy[vyr + (int64_t)j * g.nx], *v1y, g.gamma,
                            ScEnds{ly, hy, rg.recv + 4 * nyz, nxz, pry});
    acc += sc_axis<L, true>(g.c[2][k], w, k, g.nz, wz, g.kind[4], g.kind[5], g.val[4], g.val[5], g.dlo[2], g.dhi[2], prz, nxy, Vz[c], *v1z, g.gamma, ScEnds{lz, hz, rg.recv + 4 * (nyz + nxz), nxy, prz});
    if (q) acc += __builtin_nontemporal_load(q + c);
    double r = c1 * w[c] + c2 * acc;
    if (HASN) r += c0 * __builtin_nontemporal_load(phin + c);
    __builtin_nontemporal_store(r, out + c);
    // the fused pack: the next stage's exchange sends these slabs as they are
    if (rg.pack) {
      // (the lines are formed again from the row's numbers in scalar registers: kept from the top of the loop they cost six vector registers)
      const int     js = __builtin_amdgcn_readfirstlane(j), ks = __builtin_amdgcn_readfirstlane(k);
      const int64_t prx = (int64_t)ks * g.ny + js, pry = (int64_t)ks * g.nx + i, prz = (int64_t)js * g.nx + i;
      double *const sx = rg.send, *const sy = sx + 4 * nyz, *const sz = sy + 4 * nxz;
      if ((rg.pack & 1) && i < 2) sx[i * nyz + prx] = r;
      if ((rg.pack & 2) && i >= g.nx - 2) sx[(i - g.nx + 4) * nyz + prx] = r;
      if ((rg.pack & 4) && j < 2) sy[j * nxz + pry] = r;
      if ((rg.pack & 8) && j >= g.ny - 2) sy[(j - g.ny + 4) * nxz + pry] = r;
      if ((rg.pack & 16) && k < 2) sz[k * nxy + prz] = r;
      if ((rg.pack & 32) && k >= g.nz - 2) sz[(k - g.nz + 4) * nxy + prz] = r;
    }
  }
}

// The send layers of the caller's phi (the first stage of a step, fl_scalar_rhs), in the layout the fused pack writes: blockIdx.y = boundary, all six
// in one launch (a boundary without a neighbouring rank returns at once).  nl: the layers packed -- 2, or 1 for the 7-point star of
// fl_scalar_implicit.hip: the outermost cell alone, into the layer it has among the two (0 at a low end, 3 at a high end).
__global__ void __launch_bounds__(256) k_scalar_pack(int nx, int ny, int nz, int nb, int nl, const double *__restrict__ phi, double *__restrict__ send)
{
  const int b = blockIdx.y, d = b >> 1;
  if (!((nb >> b) & 1)) return;
  const int64_t nyz = (int64_t)ny * nz, nxz = (int64_t)nx * nz, nxy = (int64_t)nx * ny;
  const int     n = d == 0 ? nx : (d == 1 ? ny : nz), a0 = (b & 1) ? n - nl : 0;
  const int64_t np = d == 0 ? nyz : (d == 1 ? nxz : nxy);
  double       *out = send + (d == 0 ? 0 : (d == 1 ? 4 * nyz : 4 * (nyz + nxz))) + (b & 1 ? (4 - nl) * np : 0);
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < nl * np; t += (int64_t)gridDim.x * blockDim.x) {
    const int     a = a0 + (int)(t / np);
    const int64_t pr = t % np;
    int64_t       c;
    if (d == 0) c = pr * nx + a;                                 // pr = k ny + j
    else if (d == 1) c = ((pr / nx) * ny + a) * nx + pr % nx;   // pr = k nx + i
    else c = (int64_t)a * nxy + pr;                              // pr = j nx + i
    out[t] = phi[c];
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

// k_scalar_cfl on one rank's block of several (per: the periodic axes the rank holds alone; nb as in k_scalar_stage_ring): the face behind the last
// cell of an axis the next rank owns is read from the hiface plane vhi[d]
struct ScHiface {
  const double *v[3];
};
__global__ void __launch_bounds__(256) k_scalar_cfl_ring(int nx, int ny, int nz, int per, int nb, ScHiface vhi, double dt, double gamma, const double *__restrict__ hx,
                                                         const double *__restrict__ hy, const double *__restrict__ hz, const double *__restrict__ Vx, const double *__restrict__ Vy,
                                                         const double *__restrict__ Vz, double *__restrict__ partial)
{
  __shared__ double red[8];
  const int64_t     N = (int64_t)nx * ny * nz, nxy = (int64_t)nx * ny;
  const bool        wx = per & 1, wy = per & 2, wz = per & 4, nhx = nb & 2, nhy = nb & 8, nhz = nb & 32;
  const int         fx = (wx || nhx) ? nx : nx + 1, fy = (wy || nhy) ? ny : ny + 1;
  double            ca = 0., cd = 0.;
  for (int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x; c < N; c += (int64_t)gridDim.x * 256) {
    const int     i = (int)(c % nx);
    const int64_t t = c / nx;
    const int     j = (int)(t % ny), k = (int)(t / ny);
    const int     ip = (i + 1 == nx && wx) ? 0 : i + 1, jp = (j + 1 == ny && wy) ? 0 : j + 1, kp = (k + 1 == nz && wz) ? 0 : k + 1;
    const int64_t vxr = ((int64_t)k * ny + j) * fx, vyr = (int64_t)k * fy * nx + i;
    const double  x1 = (nhx && i + 1 == nx) ? vhi.v[0][(int64_t)k * ny + j] : Vx[vxr + ip], y1 = (nhy && j + 1 == ny) ? vhi.v[1][(int64_t)k * nx + i] : Vy[vyr + (int64_t)jp * nx],
                 z1 = (nhz && k + 1 == nz) ? vhi.v[2][(int64_t)j * nx + i] : Vz[(int64_t)kp * nxy + (int64_t)j * nx + i];
    const double ax = fmax(fabs(Vx[vxr + i]), fabs(x1)), ay = fmax(fabs(Vy[vyr + (int64_t)j * nx]), fabs(y1)), az = fmax(fabs(Vz[c]), fabs(z1));
    const double a = hx[i], b = hy[j], d = hz[k];
    ca = fmax(ca, dt * (ax / a + ay / b + az / d));
    cd = fmax(cd, gamma * dt * (2. / (a * a) + 2. / (b * b) + 2. / (d * d)));
  }
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
    partial[3 * blockIdx.x]     = 0.;
    partial[3 * blockIdx.x + 1] = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
    partial[3 * blockIdx.x + 2] = fmax(fmax(red[4], red[5]), fmax(red[6], red[7]));
  }
}

// The fluxes through the physical boundaries of the block, all (at most six) planes in one launch: the blocks first[b] .. first[b + 1] - 1 work on
// boundary b (none where the end is periodic or a neighbouring rank sits behind it), one lane per face, grid-stride within the boundary's blocks.
// partial[3 B + 1], [3 B + 2]: block B's sums of V phi_f A and of -Gamma g A, with phi_f and g of the boundary rule exactly as sc_axis forms them
// at the cells 0 and n - 1.  The x planes read V and phi with a stride of a row: a plane, not a field -- the kernel is latency-sized.
struct ScFluxPlan {
  int first[7];
};
__global__ void __launch_bounds__(256) k_scalar_flux(ScGrid g, ScFluxPlan pl, int fx, int fy, const double *__restrict__ hx, const double *__restrict__ hy, const double *__restrict__ hz,
                                                     const double *__restrict__ phi, const double *__restrict__ Vx, const double *__restrict__ Vy, const double *__restrict__ Vz,
                                                     double *__restrict__ partial)
{
  __shared__ double red[8];
  int               b = 0;
  while (b < 5 && (int)blockIdx.x >= pl.first[b + 1]) ++b;
  const int     d = b >> 1, side = b & 1, lb = blockIdx.x - pl.first[b], nlb = pl.first[b + 1] - pl.first[b];
  const int64_t nxy = (int64_t)g.nx * g.ny;
  const int     n = d == 0 ? g.nx : (d == 1 ? g.ny : g.nz), a = side ? n - 1 : 0, f = side ? n : 0;
  const int64_t np = d == 0 ? (int64_t)g.ny * g.nz : (d == 1 ? (int64_t)g.nx * g.nz : nxy);
  const ScCell  T = g.c[d][a];
  const int     kind = g.kind[b];
  const double  val = g.val[b], dist = side ? g.dhi[d] : g.dlo[d];
  double        sc = 0., sd = 0.;
  for (int64_t t = (int64_t)lb * 256 + threadIdx.x; t < np; t += (int64_t)nlb * 256) {
    int64_t c, v;
    double  A;
    const double *V;
    if (d == 0) {  // t = k ny + j
      c = t * g.nx + a, v = t * fx + f, V = Vx;
      A = hy[t % g.ny] * hz[t / g.ny];
    } else if (d == 1) {  // t = k nx + i
      const int64_t k = t / g.nx, i = t % g.nx;
      c = (k * g.ny + a) * g.nx + i, v = (k * fy + f) * g.nx + i, V = Vy;
      A = hx[i] * hz[k];
    } else {  // t = j nx + i
      c = (int64_t)a * nxy + t, v = (int64_t)f * nxy + t, V = Vz;
      A = hx[t % g.nx] * hy[t / g.nx];
    }
    const double P = phi[c];
    double       F, G;
    if (kind == 0) {
      F = val;
      G = side ? (val - P) * T.ic2 : (P - val) * T.ic1;
    } else {
      F = side ? P + dist * val : P - dist * val;
      G = val;
    }
    sc += (V[v] * F) * A;
    sd -= (g.gamma * G) * A;
  }
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    sc += __shfl_down(sc, o, 64);
    sd += __shfl_down(sd, o, 64);
  }
  if (lane == 0) {
    red[wv]     = sc;
    red[4 + wv] = sd;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    partial[3 * blockIdx.x]     = 0.;
    partial[3 * blockIdx.x + 1] = (red[0] + red[1]) + (red[2] + red[3]);
    partial[3 * blockIdx.x + 2] = (red[4] + red[5]) + (red[6] + red[7]);
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
  bool          pack;  // several ranks: the stage fills the send slabs for the stage after it
};

// a neighbouring rank behind boundary b whose cells arrive through the exchange (sv_ring_side of fl_schur_var.hip)
bool sc_ring_side(const fl_poisson *h, int b) { return h->multi && h->nbr[b] >= 0 && !h->wrap_local[b / 2]; }

ScRing ring_args(const fl_scalar *m, bool pack)
{
  ScRing rg;
  rg.recv = m->slab_recv.p;
  rg.send = m->slab_send.p;
  rg.pack = pack ? m->nb : 0;
  for (int d = 0; d < 3; ++d) rg.vhi[d] = (m->nb >> (2 * d + 1)) & 1 ? m->h->hiface[d] : nullptr;
  return rg;
}

// where the two layers of boundary b start in slab_recv / slab_send
size_t slab_offset(const fl_poisson *h, int b)
{
  size_t o = 0;
  for (int d = 0; d < b / 2; ++d) o += 4 * (size_t)fl_plane_size(h, d);
  return o + (b % 2 ? 2 * (size_t)fl_plane_size(h, b / 2) : 0);
}

template <int L>
void launch_stage(const fl_scalar *m, const StageArgs &a)
{
  const dim3 grid(8 * scalar_plan(m->g.nx, m->g.ny, m->g.nz, L).per_xcd);
  if (m->ring) {
    const ScRing rg = ring_args(m, a.pack);
    if (a.phin) hipLaunchKernelGGL((k_scalar_stage_ring<L, true>), grid, dim3(256), 0, m->h->stream, m->g, rg, m->nb, a.c0, a.c1, a.c2, a.phin, a.w, m->V[0], m->V[1], m->V[2], a.q, a.out);
    else hipLaunchKernelGGL((k_scalar_stage_ring<L, false>), grid, dim3(256), 0, m->h->stream, m->g, rg, m->nb, a.c0, a.c1, a.c2, a.phin, a.w, m->V[0], m->V[1], m->V[2], a.q, a.out);
    return;
  }
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
    // (several ranks: the periodic axes this rank holds alone -- a periodic axis split over ranks is a rank face at both ends)
    g.per |= (h->multi ? h->wrap_local[d] : A.periodic) ? 1 << d : 0;
    g.kind[2 * d] = bc[2 * d];
    g.kind[2 * d + 1] = bc[2 * d + 1];
    g.dlo[d] = A.xcc(0) - A.xf[0];
    g.dhi[d] = A.xf[(size_t)A.n] - A.xcc(A.n - 1);
    std::vector<ScCell> rows;
    FL_CHK(build_axis_scalar(A, rows));
    std::vector<double> hw((size_t)A.n);
    for (int64_t i = 0; i < A.n; ++i) hw[(size_t)i] = A.xf[(size_t)i + 1] - A.xf[(size_t)i];
    FL_CHK(m->tab[d].plain(h, (int64_t)rows.size()));
    FL_CHK(m->hw[d].plain(h, (int64_t)hw.size()));
    FL_HIP(hipMemcpy(m->tab[d].p, rows.data(), sizeof(ScCell) * rows.size(), hipMemcpyHostToDevice));
    FL_HIP(hipMemcpy(m->hw[d].p, hw.data(), sizeof(double) * hw.size(), hipMemcpyHostToDevice));
    // h->ax[d] is the GLOBAL axis: the rank's rows are the one-rank rows of its cells, bit for bit (one rank: lo = 0)
    const int64_t lo = h->multi ? h->dec.lo[d] : 0;
    g.c[d]    = m->tab[d].p + lo;
    m->hwl[d] = m->hw[d].p + lo;
  }
  FL_CHK(m->partial.plain(h, 3 * SC_REDUCE_BLOCKS));
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
  delete m;  // the DevBufs free what they hold
  return FL_SUCCESS;
}

namespace {

// the checks of the boundary kinds both constructors make, against the GLOBAL axes
int scalar_check_bc(const fl_poisson *h, const int bc[6])
{
  for (int b = 0; b < 6; ++b)
    if (bc[b] < 0 || bc[b] > 2) return FL_ERR_ARG_OUTOFRANGE;
  for (int d = 0; d < 3; ++d)
    if ((bc[2 * d] == 2) != h->ax[d].periodic || (bc[2 * d + 1] == 2) != h->ax[d].periodic) return FL_ERR_ARG_WRONG;
  return FL_SUCCESS;
}

int scalar_new(fl_poisson *h, const int bc[6], bool ring, fl_scalar **out)
{
  fl_scalar *m  = new fl_scalar();
  int        rc = scalar_init(m, h, bc);
  if (!rc && ring) {
    for (int b = 0; b < 6; ++b) m->nb |= sc_ring_side(h, b) ? 1 << b : 0;
    const int64_t n = (int64_t)slab_offset(h, 6);
    if (m->slab_recv.plain(h, n) || m->slab_send.plain(h, n)) rc = FL_ERR_GPU;
  }
  m->ring = ring;
  if (rc) {
    fl_scalar_destroy(m);
    return rc;
  }
  *out = m;
  return FL_SUCCESS;
}

// Several ranks: the phi slabs of the stage about to run, from the send layers (filled by k_scalar_pack or by the stage before) into the peers' receive
// slabs.  ONE pair of slabs per boundary is enough: the transports are stream-ordered on either side (RCCL's Send / Recv; the host-staged callbacks
// copy out of the send slab and into the receive slab on the handle's stream), so the receive of stage k + 1 is posted in stream order AFTER the
// kernel that read stage k's slab, and the kernel that overwrites a send slab after the exchange that shipped it.
// nl = 1 (scalar_ring_exchange1): the outermost layer alone -- send layer 0 / 3 of a low / high end into the peer's receive layer 2 / 1 -- under tags of
// its own (+320), so that no message of one kind can be taken for one of the other.
int ring_exchange(fl_scalar *m, int nl = 2)
{
  fl_poisson *h = m->h;
  fl_halo_msg plan[12];
  const int   np = fl_halo_messages(h, false, plan);
  const int   tag = nl == 2 ? 256 : 320;
  std::vector<Msg> msgs;
  for (int a = 0; a < np; ++a) {
    const int sb = plan[a].send_boundary, rb = plan[a].recv_boundary;
    if (!((m->nb >> sb) & 1) || !((m->nb >> rb) & 1)) return FL_ERR_ARG_WRONGSTATE;
    const size_t plane = (size_t)fl_plane_size(h, sb / 2), so = (nl == 1 && sb % 2) ? plane : 0, ro = (nl == 1 && rb % 2 == 0) ? plane : 0;
    msgs.push_back({plan[a].peer, m->slab_send + slab_offset(h, sb) + so, m->slab_recv + slab_offset(h, rb) + ro, nl * (int64_t)plane, plan[a].sendtag + tag, plan[a].recvtag + tag});
  }
  return h->comm.exchange(h->stream, msgs);
}

// the send slabs of the caller's phi: nl layers per rank face
int ring_pack(fl_scalar *m, const double *phi, int nl)
{
  size_t most = 0;
  for (int b = 0; b < 6; ++b)
    if ((m->nb >> b) & 1) most = std::max(most, nl * (size_t)fl_plane_size(m->h, b / 2));
  if (most) hipLaunchKernelGGL(k_scalar_pack, dim3((unsigned)std::min<size_t>((most + 255) / 256, 1024), 6), dim3(256), 0, m->h->stream, m->g.nx, m->g.ny, m->g.nz, m->nb, nl, phi, m->slab_send.p);
  FL_HIP(hipGetLastError());
  return FL_SUCCESS;
}

// the send slabs of the caller's phi, then the exchange
int ring_pack_exchange(fl_scalar *m, const double *phi)
{
  FL_CHK(ring_pack(m, phi, 2));
  return ring_exchange(m);
}

// what every collective call starts with: the velocity of the faces the next rank owns.  With the call, not with fl_scalar_set_velocity: the
// handle's hiface planes are shared with fl_poisson_rhs, and a plane refreshed with the call is never stale.
int ring_velocity(fl_scalar *m) { return m->ring ? fl_fill_hifaces(m->h, m->V) : 0; }

}  // namespace

extern "C" int fl_scalar_create(fl_poisson *grid_from, const int bc[6], fl_scalar **out)
{
  if (!grid_from || !bc || !out) return FL_ERR_ARG_NULL;
  *out = nullptr;
  FL_CHK(scalar_check_bc(grid_from, bc));
  if (grid_from->multi) return FL_ERR_SUP;  // one rank's block of several: fl_scalar_create_ranks (collective)
  return scalar_new(grid_from, bc, false, out);
}

extern "C" int fl_scalar_create_ranks(fl_poisson *grid_from, const int bc[6], fl_scalar **out)
{
  if (!grid_from || !bc || !out) return FL_ERR_ARG_NULL;
  if (!grid_from->multi) return fl_scalar_create(grid_from, bc, out);
  *out = nullptr;
  fl_poisson *h = grid_from;
  FL_CHK(scalar_check_bc(h, bc));
  if (h->loopback) return FL_ERR_SUP;
  if (h->comm.kind == Comm::NONE) return FL_ERR_ARG_WRONGSTATE;
  // Voted, so that every rank returns an error and none holds a handle its peers would wait for: 2 = a block with one cell along a split axis (the
  // neighbour's second layer would not be its own cell), 1 = this rank could not build its handle (tables, slabs: made BEFORE the vote)
  const int n[3] = {h->g.nx, h->g.ny, h->g.nz};
  bool      thin = false;
  for (int b = 0; b < 6; ++b)
    if (sc_ring_side(h, b) && n[b / 2] < 2) thin = true;
  FL_HIP(hipSetDevice(h->device));
  fl_scalar *m    = nullptr;
  const int  rc   = thin ? FL_SUCCESS : scalar_new(h, bc, true, &m);
  double     vote = thin ? 2. : (rc ? 1. : 0.);
  const int  vrc  = fl_allreduce_max(h, &vote);
  if (vrc || vote != 0.) {
    fl_scalar_destroy(m);
    if (vrc) return vrc;
    return vote == 2. ? FL_ERR_ARG_OUTOFRANGE : (rc ? rc : FL_ERR_GPU);
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
  if (m->ring) {
    FL_CHK(ring_velocity(m));
    FL_CHK(ring_pack_exchange(m, phi_dev));
  }
  STAGE[m->limiter](m, StageArgs{0., 0., 1., nullptr, phi_dev, source_dev, out_dev, false});
  FL_HIP(hipGetLastError());
  return FL_SUCCESS;
}

// Not part of the public C-ABI (tools/scalar_bench.py --ring): the launch of fl_scalar_rhs ALONE on a handle of fl_scalar_create_ranks -- no exchange, the
// slabs and the hiface planes as the last collective call left them -- so that one rank can time k_scalar_stage_ring while its peers idle.  pack != 0:
// the stage also fills the send slabs, as every stage of a step but the last does.
extern "C" int fldbg_scalar_stage_only(fl_scalar *m, const double *phi_dev, const double *source_dev, double *out_dev, int pack)
{
  if (!m || !phi_dev || !out_dev) return FL_ERR_ARG_NULL;
  if (phi_dev == out_dev) return FL_ERR_ARG_WRONG;
  if (!m->V[0]) return FL_ERR_ARG_WRONGSTATE;
  if (m->ring)
    for (int d = 0; d < 3; ++d)
      if (((m->nb >> (2 * d + 1)) & 1) && !m->h->hiface[d]) return FL_ERR_ARG_WRONGSTATE;  // (no collective call yet)
  FL_HIP(hipSetDevice(m->h->device));
  STAGE[m->limiter](m, StageArgs{0., 0., 1., nullptr, phi_dev, source_dev, out_dev, m->ring && pack != 0});
  FL_HIP(hipGetLastError());
  return FL_SUCCESS;
}

// w <- phi; s - 1 times w <- w + dt / (s - 1) R(w); phi <- ((s - 1) w + phi + dt R(w)) / s.  One launch per stage; the stage vectors alternate between
// the handle's two work arrays, and the last stage writes phi in place (it reads of phi only the cell it writes) -- or, for fl_scalar_step_imex, into
// an array of the handle's.
// Not part of the public C-ABI (tests): every word of both slabs of a handle of fl_scalar_create_ranks becomes a NaN (all bits set), in stream order -- a call
// that read a layer it had not received or packed itself would show it
extern "C" int fldbg_scalar_poison_slabs(fl_scalar *m)
{
  if (!m) return FL_ERR_ARG_NULL;
  if (!m->ring) return FL_ERR_SUP;
  FL_HIP(hipSetDevice(m->h->device));
  const size_t bytes = sizeof(double) * slab_offset(m->h, 6);
  if (bytes) {
    FL_HIP(hipMemsetAsync(m->slab_recv, 0xFF, bytes, m->h->stream));
    FL_HIP(hipMemsetAsync(m->slab_send, 0xFF, bytes, m->h->stream));
  }
  return FL_SUCCESS;
}

int fl::scalar_ring_pack1(fl_scalar *m, const double *phi_dev) { return ring_pack(m, phi_dev, 1); }
int fl::scalar_ring_exchange1(fl_scalar *m) { return ring_exchange(m, 1); }

int fl::scalar_ssp_step(fl_scalar *m, double dt, int nstages, const double *source_dev, const double *phi_dev, double *out_dev, bool pack_last)
{
  FL_HIP(hipSetDevice(m->h->device));
  for (int a = 0; a < (nstages > 2 ? 2 : 1); ++a)
    if (!m->work[a]) FL_CHK(m->work[a].plain(m->h, m->h->ncell));
  const int     s = nstages;
  const double *w = phi_dev;
  // several ranks: V is frozen during the step (one exchange of its high faces); phi's slabs are packed by a kernel once, then by the stages
  if (m->ring) {
    FL_CHK(ring_velocity(m));
    FL_CHK(ring_pack_exchange(m, phi_dev));
  }
  for (int st = 0; st < s - 1; ++st) {
    double *o = m->work[st & 1];
    STAGE[m->limiter](m, StageArgs{0., 1., dt / (s - 1), nullptr, w, source_dev, o, m->ring});
    if (m->ring) FL_CHK(ring_exchange(m));
    w = o;
  }
  STAGE[m->limiter](m, StageArgs{1. / s, (s - 1.) / s, dt / s, phi_dev, w, source_dev, out_dev, m->ring && pack_last});
  FL_HIP(hipGetLastError());
  return FL_SUCCESS;
}

extern "C" int fl_scalar_step(fl_scalar *m, double dt, int nstages, const double *source_dev, double *phi_dev)
{
  if (!m || !phi_dev) return FL_ERR_ARG_NULL;
  if (nstages < 2 || !std::isfinite(dt)) return FL_ERR_ARG_OUTOFRANGE;
  if (!m->V[0]) return FL_ERR_ARG_WRONGSTATE;
  return scalar_ssp_step(m, dt, nstages, source_dev, phi_dev, phi_dev, false);
}

extern "C" int fl_scalar_cfl(fl_scalar *m, double dt, double out[2])
{
  if (!m || !out) return FL_ERR_ARG_NULL;
  if (!m->V[0]) return FL_ERR_ARG_WRONGSTATE;
  FL_HIP(hipSetDevice(m->h->device));
  const int nb = reduce_blocks(m);
  if (m->ring) {
    FL_CHK(ring_velocity(m));
    ScHiface vh;
    for (int d = 0; d < 3; ++d) vh.v[d] = (m->nb >> (2 * d + 1)) & 1 ? m->h->hiface[d] : nullptr;
    hipLaunchKernelGGL(k_scalar_cfl_ring, dim3(nb), dim3(256), 0, m->h->stream, m->g.nx, m->g.ny, m->g.nz, m->g.per, m->nb, vh, dt, m->g.gamma, m->hwl[0], m->hwl[1], m->hwl[2], m->V[0],
                       m->V[1], m->V[2], m->partial.p);
  } else
    hipLaunchKernelGGL(k_scalar_cfl, dim3(nb), dim3(256), 0, m->h->stream, m->g.nx, m->g.ny, m->g.nz, m->g.per, dt, m->g.gamma, m->hwl[0], m->hwl[1], m->hwl[2], m->V[0], m->V[1], m->V[2],
                       m->partial.p);
  FL_CHK(fetch_partials(m, nb));
  out[0] = out[1] = 0.;
  for (int b = 0; b < nb; ++b) {
    out[0] = std::max(out[0], m->partial_host[(size_t)3 * b + 1]);
    out[1] = std::max(out[1], m->partial_host[(size_t)3 * b + 2]);
  }
  if (m->ring) {  // a maximum is the same number in any order: the same bits on every rank and every rank grid
    FL_CHK(fl_allreduce_max(m->h, &out[0]));
    FL_CHK(fl_allreduce_max(m->h, &out[1]));
  }
  return FL_SUCCESS;
}

extern "C" int fl_scalar_stats(fl_scalar *m, const double *phi_dev, double out[3])
{
  if (!m || !phi_dev || !out) return FL_ERR_ARG_NULL;
  FL_HIP(hipSetDevice(m->h->device));
  const int nb = reduce_blocks(m);
  hipLaunchKernelGGL(k_scalar_stats, dim3(nb), dim3(256), 0, m->h->stream, m->g.nx, m->g.ny, m->g.nz, m->hwl[0], m->hwl[1], m->hwl[2], phi_dev, m->partial.p);
  FL_CHK(fetch_partials(m, nb));
  out[0] = m->partial_host[0];
  out[1] = m->partial_host[1];
  out[2] = 0.;
  for (int b = 0; b < nb; ++b) {
    out[0] = std::min(out[0], m->partial_host[(size_t)3 * b]);
    out[1] = std::max(out[1], m->partial_host[(size_t)3 * b + 1]);
    out[2] += m->partial_host[(size_t)3 * b + 2];
  }
  if (m->ring) {  // min as the negated maximum; the sum: the ranks' block-ordered sums added in the all-reduce's fixed order
    double neg = -out[0];
    FL_CHK(fl_allreduce_max(m->h, &neg));
    out[0] = -neg;
    FL_CHK(fl_allreduce_max(m->h, &out[1]));
    FL_CHK(fl_allreduce_sum(m->h, &out[2]));
  }
  return FL_SUCCESS;
}

// One launch over the boundary planes, at most SC_FLUX_BLOCKS blocks per boundary (their partial sums share the handle's slab with the other
// reductions), the blocks of a boundary added in block order on the host.
constexpr int SC_FLUX_BLOCKS = 64;
extern "C" int fl_scalar_boundary_flux(fl_scalar *m, const double *phi_dev, double out[12])
{
  if (!m || !phi_dev || !out) return FL_ERR_ARG_NULL;
  if (!m->V[0]) return FL_ERR_ARG_WRONGSTATE;
  static_assert(6 * SC_FLUX_BLOCKS <= SC_REDUCE_BLOCKS, "the partial sums of six boundaries fit the slab");
  FL_HIP(hipSetDevice(m->h->device));
  const ScGrid &g = m->g;
  ScFluxPlan    pl;
  pl.first[0] = 0;
  for (int b = 0; b < 6; ++b) {
    // a physical boundary of THIS block: not periodic, and no neighbouring rank behind it
    const bool    physical = g.kind[b] != 2 && !((m->nb >> b) & 1);
    const int64_t np = fl_plane_size(m->h, b / 2);
    pl.first[b + 1] = pl.first[b] + (physical ? (int)std::min<int64_t>((np + 255) / 256, SC_FLUX_BLOCKS) : 0);
  }
  for (int a = 0; a < 12; ++a) out[a] = 0.;
  const int nblk = pl.first[6];
  if (nblk) {
    const bool hx = (m->nb >> 1) & 1, hy = (m->nb >> 3) & 1;
    const int  fx = ((g.per & 1) || hx) ? g.nx : g.nx + 1, fy = ((g.per & 2) || hy) ? g.ny : g.ny + 1;
    hipLaunchKernelGGL(k_scalar_flux, dim3(nblk), dim3(256), 0, m->h->stream, g, pl, fx, fy, m->hwl[0], m->hwl[1], m->hwl[2], phi_dev, m->V[0], m->V[1], m->V[2], m->partial.p);
    FL_CHK(fetch_partials(m, nblk));
    for (int b = 0; b < 6; ++b)
      for (int k = pl.first[b]; k < pl.first[b + 1]; ++k) {
        out[2 * b] += m->partial_host[(size_t)3 * k + 1];
        out[2 * b + 1] += m->partial_host[(size_t)3 * k + 2];
      }
  } else
    FL_HIP(hipStreamSynchronize(m->h->stream));
  if (m->ring) {  // (the all-reduce carries eight numbers at a time)
    FL_CHK(fl_poisson_allreduce_sum(m->h, out, 8));
    FL_CHK(fl_poisson_allreduce_sum(m->h, out + 8, 4));
  }
  return FL_SUCCESS;
}
