// fl_ibm.hip -- immersed-boundary delta-function interpolation / spreading.
//
// There is NO reference implementation (thecasterian/fluca THEORY_GUIDE.md:130-132 is an empty TODO); the specification
// is DESIGN.md "IBM":  U_l = sum_x u(x) delta_h(x - X_l) h^3,  f(x) += sum_l F_l delta_h(x - X_l) dV_l,
// delta_h = prod_d phi(r_d / h_d) / h_d, phi = Peskin 4-point or Roma 3-point, collocated fields (all velocity components live
// at cell centres in Fluca, fluca/src/ns/interface/nsbasic.c:180) so one weight set serves every component.
// Stretched axes (round 2): the delta function lives in INDEX space -- the marker is mapped to the continuous cell-centre index s
// (piecewise linear through the centres; beyond the first / last one through its mirror image in the wall or the periodic image),
// the weights are phi(s - i), interpolation is U = sum u w and spreading divides by the volume of the TARGET cell:
// f_i += F dV w / (dx_i dy_j dz_k).  sum w = 1, <interp u, F dV> = sum_i u_i f_i V_i and sum_i f_i V_i = sum F dV hold on any
// grid; on a uniform one this is exactly the formula above.
//
// Kernels (gfx950, 64-lane wavefronts):
//   k_ibm_weights   one lane per marker: first support cell and the S 1-D weights per axis
//   k_ibm_interp    ONE WAVEFRONT PER MARKER, one lane per support cell (4^3 = 64 lanes exactly), fixed-order wave
//                   reduction -> deterministic
//   k_ibm_spread    gather form, no atomics: one 256-thread block per 8x8x8 tile of cells; the markers whose support
//                   touches the tile (per-tile bins built at create/update) are staged in LDS, rank-sorted by marker id
//                   in LDS so that every cell accumulates in a run-independent order -> bitwise reproducible
//
// Several ranks, two ways to hold the markers:
//   replicated (fl_ibm_create)        every rank holds all L markers; interp ends in an all-reduce of ncomp L doubles
//   owner rank (fl_ibm_create_owned)  a marker lives on the rank that owns the cell nearest to it; where its support reaches into a
//                                     neighbouring block, that neighbour holds a GHOST COPY of the marker (position and id, exchanged at
//                                     create / update).  Both ranks run the kernels above over own + ghost markers on their own cells;
//                                     interp returns the ghosts' partial sums to the owners, spread sends F and dV of the copies out.
//                                     No field and no all-reduce is involved: (ghost copies) x 24-32 bytes per call.
// fl_ibm_owner.hip:
//   k_ibm_route     one lane per own marker: is its cell in this block, and which of the 26 neighbour offsets does its support reach
//   k_ibm_pack_pos / k_ibm_unpack_pos, k_ibm_pack_U, k_ibm_collect_U, k_ibm_pack_F, k_ibm_stage_F
//                   one lane per copy / ghost / marker: records of the messages through the send list, and the owners' sums in
//                   ascending offset code (a fixed order: deterministic)
//   migration (fl_ibm_migrate): a marker whose owner cell has moved into a neighbouring block goes there with position, number and attributes
//   k_ibm_dest      one lane per own marker: the offset code of its new owner (13: it stays), the 27 counts by ballot and popcount per wave
//   k_ibm_split     stayers compacted in order (ballot scan per block + block offsets), leavers packed as records per offset
//   k_ibm_rank_arrivals, k_ibm_merge
//                   arrivals ranked by number (counting, tiled through LDS), then stayers and arrivals -- both ascending -- into one ascending
//                   list by binary search in each other's numbers: the own list of a set created afresh, without a sort
// here again:
//   k_ibm_rigid_pose  a rigid body's markers and target velocities from their reference positions (the host mirror's moving body)
// fl_ibm_body.hip:
//   k_ibm_force_max, k_ibm_force_sum  force and torque on each body as sums whose bits depend on no order (fl_ibm_force)
//   a scalar held on the markers (fl_ibm_scalar_force, include/fluca_hip_ibm_scalar.h): per pass the bits of interp(1), T - Phi, spread(1)
//   k_ibm_scalar_defect  k_ibm_interp for one field whose lane 0 goes on to q = T - Phi and the running Q (one rank: the defect in the interpolation's launch)
//   k_ibm_scalar_q       one lane per own marker: q and Q from a Phi that is complete (behind k_ibm_collect_U / the all-reduce)
//   k_ibm_spread<1>      (here) the spread's one-component instantiation: one staged value per marker, two accumulators per thread
#include "fl_ibm_handle.h"

namespace fl {

// i0[d*L + l] = first support cell (GLOBAL index; beyond a wall out of range, on a periodic axis in [0, ng)); w[(d*4 + a)*L + l] = phi weights
__global__ void k_ibm_weights(IbmP P, const double *__restrict__ X, const double *__restrict__ Y, const double *__restrict__ Z, int *__restrict__ i0, double *__restrict__ w)
{
  const int64_t l = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (l >= P.L) return;
  const double pos[3] = {X[l], Y[l], Z[l]};
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    const double s = ibm_index(P, d, pos[d]);  // position in units of the cell-centre index
    const int    i = ibm_first(P, s);
    for (int a = 0; a < 4; ++a) {
      const double r          = s - (double)(i + a);
      w[(d * 4 + a) * P.L + l] = a < P.S ? (P.kind == FL_DELTA_PESKIN4 ? phi_peskin4(r) : phi_roma3(r)) : 0.;
    }
    i0[d * P.L + l] = ibm_wrap_first(P, d, i);
  }
}

// pass 0: cnt[tile]++ ; pass 1: list[off[tile] + cursor[tile]++] = marker
__global__ void k_ibm_bin(IbmP P, const int *__restrict__ i0, int *__restrict__ cnt, const int *__restrict__ off, int *__restrict__ list, int pass)
{
  const int64_t l = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (l >= P.L) return;
  int tx[4], ty[4], tz[4];
  const int nx = support_tiles(P, 0, i0[l], tx), ny = support_tiles(P, 1, i0[P.L + l], ty), nz = support_tiles(P, 2, i0[2 * P.L + l], tz);
  for (int c = 0; c < nz; ++c)
    for (int b = 0; b < ny; ++b)
      for (int a = 0; a < nx; ++a) {
        const int tile = (tz[c] * P.nt[1] + ty[b]) * P.nt[0] + tx[a];
        const int pos  = atomicAdd(&cnt[tile], 1);
        if (pass) list[off[tile] + pos] = (int)l;
      }
}

// exclusive scan of cnt[0..n) -> off[0..n], single block
__global__ void __launch_bounds__(256) k_ibm_scan(const int *__restrict__ cnt, int *__restrict__ off, int n)
{
  __shared__ int part[256];
  __shared__ int carry;
  if (threadIdx.x == 0) carry = 0;
  __syncthreads();
  for (int base = 0; base < n; base += 256 * 16) {
    int loc[16], sum = 0;
    for (int a = 0; a < 16; ++a) {
      const int idx = base + threadIdx.x * 16 + a;
      loc[a]        = idx < n ? cnt[idx] : 0;
      sum += loc[a];
    }
    part[threadIdx.x] = sum;
    __syncthreads();
    // Hillis-Steele inclusive scan over the 256 per-thread sums
    for (int o = 1; o < 256; o <<= 1) {
      const int v = (int)threadIdx.x >= o ? part[threadIdx.x - o] : 0;
      __syncthreads();
      part[threadIdx.x] += v;
      __syncthreads();
    }
    int run = carry + part[threadIdx.x] - sum;
    for (int a = 0; a < 16; ++a) {
      const int idx = base + threadIdx.x * 16 + a;
      if (idx < n) off[idx] = run;
      run += loc[a];
    }
    __syncthreads();
    if (threadIdx.x == 255) carry += part[255];
    __syncthreads();
  }
  if (threadIdx.x == 0) off[n] = carry;
}

// U[c*L + l] = sum over the support.  One wavefront per marker, lane = (a,b,c3) of the S^3 support.
__global__ void __launch_bounds__(256) k_ibm_interp(IbmP P, const int *__restrict__ i0, const double *__restrict__ w, int ncomp, int64_t ncell, const double *__restrict__ u, double *__restrict__ U)
{
  const int     lane = threadIdx.x & 63;
  const int64_t l    = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (l >= P.L) return;
  const int S = P.S;
  const int a = lane % S, b = (lane / S) % S, c3 = lane / (S * S);
  double    wt   = 0.;
  int64_t   cell = -1;
  if (c3 < S) {
    const int ci = support_cell(P, 0, i0[l], a), cj = support_cell(P, 1, i0[P.L + l], b), ck = support_cell(P, 2, i0[2 * P.L + l], c3);
    if (ci >= 0 && cj >= 0 && ck >= 0) {
      cell = ((int64_t)ck * P.n[1] + cj) * P.n[0] + ci;
      wt   = w[(0 * 4 + a) * P.L + l] * w[(1 * 4 + b) * P.L + l] * w[(2 * 4 + c3) * P.L + l];
    }
  }
  for (int c = 0; c < ncomp; ++c) {
    double v = cell >= 0 ? wt * u[(int64_t)c * ncell + cell] : 0.;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    if (lane == 0) U[(int64_t)c * P.L + l] = v;
  }
}

// f[c*ncell + x] += sum_l w_l(x) F[c*L + l] dV_l / (hx hy hz), gather over the tile's bin, markers in ascending id order.
// A loop that looks every marker's weights up (its first cell -> the index into its weights -> the weight) is a chain of dependent LDS reads behind two
// divergent tests, one wave per SIMD and block: about 300 cycles per marker and 150 markers per bin of config 4's sphere.  Here the staging step expands
// every marker's 1-D weights onto the tile's eight cells per axis (zero outside the support, periodic wrap and all), so the loop reads four weights and
// three forces at addresses that depend on nothing but the thread and the loop counter -- no test, no dependent read, unrolled.  A cell outside a marker's
// support adds an exact zero, so the sums (ascending marker id per cell) are the same bits as that loop's.
// NC: components staged and accumulated per cell.  3 is the launch of fl_ibm_spread (ncomp <= 3 at run time); 1 is the scalar forcing's: one staged
// value per marker and two accumulators per thread instead of three and six, the same operations per component.
template <int NC>
__global__ void __launch_bounds__(256) k_ibm_spread(IbmP P, const int *__restrict__ i0, const double *__restrict__ w, const int *__restrict__ off, const int *__restrict__ list, const int *__restrict__ active, int ncomp, int64_t ncell, const double *__restrict__ F,
                                                    const double *__restrict__ dV, double *__restrict__ f)
{
  __shared__ double swl[3][BIN_CHUNK][TB];  // weight of marker e on the tile's cell c of axis d
  __shared__ double sF[NC][BIN_CHUNK];
  const int tile = active[blockIdx.x];  // only tiles with a non-empty bin are launched
  const int beg = off[tile], end = off[tile + 1];
  if (beg == end) return;
  const int tt[3] = {tile % P.nt[0], (tile / P.nt[0]) % P.nt[1], tile / (P.nt[0] * P.nt[1])};
  const bool   uni = P.uniform[0] && P.uniform[1] && P.uniform[2];
  const double ih  = uni ? 1. / (P.h[0] * P.h[1] * P.h[2]) : 1.;  // stretched grids: 1 / (volume of the target cell), applied per cell below
  // this thread's two cells: (ci, cj, ck) and (ci, cj, ck + 4)
  const int li = threadIdx.x & 7, lj = (threadIdx.x >> 3) & 7, lk = threadIdx.x >> 6;
  const int ci = tt[0] * TB + li, cj = tt[1] * TB + lj;
  double    acc[2][NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) acc[0][c] = acc[1][c] = 0.;
  for (int c0 = beg; c0 < end; c0 += BIN_CHUNK) {  // bins are sorted by marker id (k_ibm_sort_bins): chunks in list order keep the order
    const int n = min(BIN_CHUNK, end - c0);
    __syncthreads();
    if ((int)threadIdx.x < n) {
      const int m = list[c0 + threadIdx.x];
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        const int first = i0[d * P.L + m];
        double    wd[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) wd[a] = w[(d * 4 + a) * P.L + m];
#pragma unroll
        for (int c = 0; c < TB; ++c) {
          int a = tt[d] * TB + c + P.lo[d] - first;
          if (P.periodic[d]) { if (a < 0) a += P.ng[d]; else if (a >= P.ng[d]) a -= P.ng[d]; }
          swl[d][threadIdx.x][c] = (a < 0 || a >= P.S) ? 0. : (a == 0 ? wd[0] : (a == 1 ? wd[1] : (a == 2 ? wd[2] : wd[3])));
        }
      }
      const double dv = dV[m] * ih;
#pragma unroll
      for (int c = 0; c < NC; ++c) sF[c][threadIdx.x] = c < ncomp ? F[(int64_t)c * P.L + m] * dv : 0.;
    }
    __syncthreads();
#pragma unroll 4
    for (int e = 0; e < n; ++e) {
      const double wxy = swl[0][e][li] * swl[1][e][lj];
      const double wt0 = wxy * swl[2][e][lk], wt1 = wxy * swl[2][e][lk + 4];
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        const double fc = sF[c][e];
        acc[0][c] += wt0 * fc;
        acc[1][c] += wt1 * fc;
      }
    }
  }
  if (ci < P.n[0] && cj < P.n[1])
    for (int half = 0; half < 2; ++half) {
      const int ck = tt[2] * TB + lk + 4 * half;
      if (ck >= P.n[2]) continue;
      const int64_t cell = ((int64_t)ck * P.n[1] + cj) * P.n[0] + ci;
      const double  vinv = uni ? 1. : P.idx[0][ci] * P.idx[1][cj] * P.idx[2][ck];
#pragma unroll
      for (int c = 0; c < NC; ++c)
        if (c < ncomp && acc[half][c] != 0.) f[(int64_t)c * ncell + cell] += acc[half][c] * vinv;
    }
}

// compact list of the tiles whose bin is not empty (order irrelevant: every tile owns its cells)
__global__ void k_ibm_active(const int *__restrict__ off, int ntiles, int *__restrict__ active, int *__restrict__ nactive)
{
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < ntiles && off[t + 1] > off[t]) active[atomicAdd(nactive, 1)] = t;
}

// in-place ascending sort of every bin by marker id: rank sort, one block per tile.  The id is the list index (replicated markers,
// unique within a bin) or, for owner-rank markers, the caller's global number gid[] (ties, which a caller's duplicate numbers would
// make, fall back to the list index) -- so that a cell adds the same markers in the same order however they are shared out.
__global__ void __launch_bounds__(256) k_ibm_sort_bins(const int *__restrict__ off, int *__restrict__ list, int *__restrict__ scratch, const int *__restrict__ active, const int64_t *__restrict__ gid)
{
  const int tile = active[blockIdx.x];
  const int beg = off[tile], end = off[tile + 1], n = end - beg;
  if (n <= 1) return;
  for (int e = threadIdx.x; e < n; e += 256) {
    const int v = list[beg + e];
    int       rank = 0;
    if (!gid)
      for (int o = 0; o < n; ++o) rank += list[beg + o] < v;
    else {
      const int64_t kv = gid[v];
      for (int o = 0; o < n; ++o) {
        const int     u  = list[beg + o];
        const int64_t ku = gid[u];
        rank += (ku < kv) || (ku == kv && u < v);
      }
    }
    scratch[beg + rank] = v;
  }
  __syncthreads();
  for (int e = threadIdx.x; e < n; e += 256) list[beg + e] = scratch[beg + e];
}

// ---- a body in prescribed rigid motion (fl_ibm_rigid_pose) -----------------------------------------------------------------------------
struct PoseP {
  double c0[3], c[3], R[9], v[3], w[3];  // reference centre, centre now, rotation matrix (row-major), velocity of the centre, angular velocity
};
// X = c + R (X0 - c0);  Ut = v + w x (X - c), Ut[c*L + l].  Either output may be absent.
__global__ void k_ibm_rigid_pose(int64_t L, PoseP P, const double *__restrict__ X0, const double *__restrict__ Y0, const double *__restrict__ Z0, double *__restrict__ X, double *__restrict__ Y, double *__restrict__ Z, double *__restrict__ Ut)
{
  const int64_t l = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (l >= L) return;
  const double r0[3] = {X0[l] - P.c0[0], Y0[l] - P.c0[1], Z0[l] - P.c0[2]};
  double       r[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) r[a] = P.R[3 * a] * r0[0] + P.R[3 * a + 1] * r0[1] + P.R[3 * a + 2] * r0[2];
  if (X) {
    X[l] = P.c[0] + r[0];
    Y[l] = P.c[1] + r[1];
    Z[l] = P.c[2] + r[2];
  }
  if (Ut) {
    Ut[l]         = P.v[0] + (P.w[1] * r[2] - P.w[2] * r[1]);
    Ut[L + l]     = P.v[1] + (P.w[2] * r[0] - P.w[0] * r[2]);
    Ut[2 * L + l] = P.v[2] + (P.w[0] * r[1] - P.w[1] * r[0]);
  }
}

}  // namespace fl

// ---- the launches the other units share ---------------------------------------------------------------------------------------------------

void ibm_launch_interp(fl_ibm *m, int64_t L, int ncomp, const double *u, double *U)
{
  hipLaunchKernelGGL(k_ibm_interp, dim3((unsigned)((L + 3) / 4)), dim3(256), 0, m->gp->stream, m->P, m->i0, m->w, ncomp, m->gp->ncell, u, U);
}

void ibm_launch_spread(fl_ibm *m, int ncomp, const double *F, const double *dV, double *f, bool one)
{
  fl_poisson *h = m->gp;
  if (m->nactive > 0 && one) hipLaunchKernelGGL(k_ibm_spread<1>, dim3(m->nactive), dim3(256), 0, h->stream, m->P, m->i0, m->w, m->off, m->list, m->active, 1, h->ncell, F, dV, f);
  else if (m->nactive > 0) hipLaunchKernelGGL(k_ibm_spread<3>, dim3(m->nactive), dim3(256), 0, h->stream, m->P, m->i0, m->w, m->off, m->list, m->active, ncomp, h->ncell, F, dV, f);
}

void ibm_launch_scan(hipStream_t s, const int *cnt, int *off, int n) { hipLaunchKernelGGL(k_ibm_scan, dim3(1), dim3(256), 0, s, cnt, off, n); }

// ---- the marker set -------------------------------------------------------------------------------------------------------------------------

int ibm_rebin(fl_ibm *m)
{
  fl_poisson *h = m->gp;
  hipStream_t s = h->stream;
  const IbmP &P = m->P;
  m->nactive    = 0;
  if (P.L == 0) return 0;  // a rank that owns no marker and holds no ghost
  const int   nb = (int)((P.L + 255) / 256);
  hipLaunchKernelGGL(k_ibm_weights, dim3(nb), dim3(256), 0, s, P, m->X, m->Y, m->Z, m->i0, m->w);
  FL_HIP(hipMemsetAsync(m->cnt, 0, sizeof(int) * (m->ntiles + 1), s));
  hipLaunchKernelGGL(k_ibm_bin, dim3(nb), dim3(256), 0, s, P, m->i0, m->cnt, m->off, m->list, 0);
  ibm_launch_scan(s, m->cnt, m->off, m->ntiles);
  FL_HIP(hipMemsetAsync(m->cnt, 0, sizeof(int) * (m->ntiles + 1), s));
  hipLaunchKernelGGL(k_ibm_bin, dim3(nb), dim3(256), 0, s, P, m->i0, m->cnt, m->off, m->list, 1);
  FL_HIP(hipMemsetAsync(m->nact_dev, 0, sizeof(int), s));
  hipLaunchKernelGGL(k_ibm_active, dim3((m->ntiles + 255) / 256), dim3(256), 0, s, m->off, m->ntiles, m->active, m->nact_dev);
  FL_HIP(hipMemcpyAsync(&m->nactive, m->nact_dev, sizeof(int), hipMemcpyDeviceToHost, s));
  FL_HIP(hipStreamSynchronize(s));  // set-up time only (create / marker update), never inside interp / spread
  // sort only the non-empty bins (ascending marker id -> run-independent accumulation order)
  if (m->nactive > 0) hipLaunchKernelGGL(k_ibm_sort_bins, dim3(m->nactive), dim3(256), 0, s, m->off, m->list, m->scratch, m->active, (const int64_t *)(m->has_gid ? m->gid.p : nullptr));
  FL_HIP(hipGetLastError());
  return 0;
}

// the per-marker group for L markers (own + ghost of an owner-rank set: the number changes with every update)
int ibm_alloc_markers(fl_ibm *m, int64_t L)
{
  fl_poisson *h = m->gp;
  if (L <= m->cap) return 0;
  // the whole group is released before any of it is allocated: every wait and free meets a stream that holds none of the new arrays' memsets
  m->X.release(h), m->Y.release(h), m->Z.release(h), m->w.release(h), m->i0.release(h), m->list.release(h), m->scratch.release(h), m->gid.release(h);
  m->listcap =(int)std::min<int64_t>(L * 27, (int64_t)1 << 30);
  int rc     = 0;
  rc |= m->X.exact(h, L, false);
  rc |= m->Y.exact(h, L, false);
  rc |= m->Z.exact(h, L, false);
  rc |= m->w.exact(h, 12 * L, false);
  rc |= m->i0.exact(h, 3 * L, false);
  rc |= m->list.exact(h, m->listcap, true);
  rc |= m->scratch.exact(h, m->listcap, true);
  if (m->owned) rc |= m->gid.exact(h, L, true);
  if (rc) return FL_ERR_MEM;
  m->cap = L;
  return 0;
}

// grid, block and delta function of a marker set; xcg[d] receives the device copy of a stretched axis' centres
int ibm_geometry(fl_poisson *h, int kind, IbmP &P, DevBuf<double> xcg[3])
{
  P.kind = kind;
  P.S    = kind == FL_DELTA_PESKIN4 ? 4 : 3;
  P.L    = 0;
  for (int d = 0; d < 3; ++d) {
    const Axis &A = h->ax[d];
    P.n[d]        = (int)h->dec.len[d];
    P.lo[d]       = (int)h->dec.lo[d];
    P.ng[d]       = (int)A.n;
    P.periodic[d] = A.periodic ? 1 : 0;
    P.x0[d]       = A.xf[0];
    P.h[d]        = (A.xf[A.n] - A.xf[0]) / (double)A.n;
    P.uniform[d]  = 1;
    for (int64_t i = 0; i < A.n; ++i)
      if (std::fabs((A.xf[i + 1] - A.xf[i]) - P.h[d]) > 1e-10 * P.h[d]) P.uniform[d] = 0;
    P.xcg[d] = nullptr;
    P.idx[d] = h->g.idx[d];
    if (!P.uniform[d]) {
      // extended centres, index -1..n: the periodic images (stored by build_axis) or the mirror images in the walls
      std::vector<double> xc((size_t)A.n + 2);
      for (int64_t i = -1; i <= A.n; ++i) xc[(size_t)(i + 1)] = A.xcc(i);
      if (!A.periodic) {
        xc[0]                  = 2. * A.xf[0] - A.xcc(0);
        xc[(size_t)A.n + 1]    = 2. * A.xf[A.n] - A.xcc(A.n - 1);
      }
      if (xcg[d].exact(h, (int64_t)xc.size(), false) || hipMemcpy(xcg[d], xc.data(), sizeof(double) * xc.size(), hipMemcpyHostToDevice) != hipSuccess) return FL_ERR_GPU;
      P.xcg[d] = xcg[d] + 1;
    }
    if (P.periodic[d] && P.ng[d] < 2 * P.S) return FL_ERR_ARG_OUTOFRANGE;
    P.nt[d] = (P.n[d] + TB - 1) / TB;
  }
  return 0;
}

int ibm_new(fl_poisson *h, int kind, bool owned, fl_ibm **out)
{
  fl_ibm *m = new fl_ibm();
  m->gp     = h;
  m->owned  = owned;
  int rc    = ibm_geometry(h, kind, m->P, m->xcg);
  if (!rc) {
    const IbmP &P = m->P;
    m->ntiles     = P.nt[0] * P.nt[1] * P.nt[2];
    int bad       = 0;
    bad |= m->cnt.exact(h, m->ntiles + 1, true);
    bad |= m->off.exact(h, m->ntiles + 1, true);
    bad |= m->active.exact(h, m->ntiles, true);
    bad |= m->nact_dev.exact(h, 1, true);
    if (bad) rc = FL_ERR_MEM;
  }
  if (rc) {
    fl_ibm_destroy(m);
    return rc;
  }
  *out = m;
  return 0;
}

extern "C" int fl_ibm_create(fl_poisson *h, int kind, int64_t L, const double *X, const double *Y, const double *Z, fl_ibm **out)
{
  if (!h || !X || !Y || !Z || !out) return FL_ERR_ARG_NULL;
  FL_CHK(ibm_check_kind_count(kind, L));
  *out = nullptr;
  FL_HIP(hipSetDevice(h->device));
  fl_ibm *m = nullptr;
  FL_CHK(ibm_new(h, kind, false, &m));
  m->P.L = L;
  if (ibm_alloc_markers(m, L)) {
    fl_ibm_destroy(m);
    return FL_ERR_MEM;
  }
  *out = m;
  return fl_ibm_update(m, X, Y, Z);
}

extern "C" int fl_ibm_update(fl_ibm *m, const double *X, const double *Y, const double *Z)
{
  if (!m) return FL_ERR_ARG_NULL;
  fl_poisson *h = m->gp;
  if (m->owned) {
    FL_HIP(hipSetDevice(h->device));
    double    v   = (m->Lo > 0 && (!X || !Y || !Z)) ? 1. : 0.;
    const int vrc = ibm_vote(h, &v, 1);
    if (vrc) return vrc;
    if (v > 0.) return (m->Lo > 0 && (!X || !Y || !Z)) ? FL_ERR_ARG_NULL : FL_ERR_ARG_OUTOFRANGE;
    return ibm_route(m, m->Lo, X, Y, Z, nullptr, false);
  }
  if (!X || !Y || !Z) return FL_ERR_ARG_NULL;
  FL_HIP(hipSetDevice(h->device));
  FL_CHK(ibm_copy_xyz(h->stream, (size_t)m->P.L, m->X, m->Y, m->Z, X, Y, Z));
  return ibm_rebin(m);
}

extern "C" int fl_ibm_interp(fl_ibm *m, int ncomp, const double *u, double *U)
{
  if (!m || !u) return FL_ERR_ARG_NULL;
  if (ncomp < 1) return FL_ERR_ARG_OUTOFRANGE;
  fl_poisson *h = m->gp;
  FL_HIP(hipSetDevice(h->device));
  if (m->owned) return ibm_interp_owned(m, ncomp, u, U);
  if (!U) return FL_ERR_ARG_NULL;
  ibm_launch_interp(m, m->P.L, ncomp, u, U);
  FL_HIP(hipGetLastError());
  // multi-rank: every rank summed over the support cells it owns; the marker value is the sum over ranks
  if (h->multi) {
    if (h->comm.kind == Comm::NONE) return FL_ERR_ARG_WRONGSTATE;
    FL_CHK(h->comm.allreduce(h->stream, U, (int)(m->P.L * ncomp)));
  }
  return FL_SUCCESS;
}

extern "C" int fl_ibm_spread(fl_ibm *m, int ncomp, const double *F, const double *dV, double *f)
{
  if (!m || !f) return FL_ERR_ARG_NULL;
  if (ncomp < 1 || ncomp > 3) return FL_ERR_ARG_OUTOFRANGE;
  fl_poisson *h = m->gp;
  FL_HIP(hipSetDevice(h->device));
  if (m->owned) return ibm_spread_owned(m, ncomp, F, dV, f);
  if (!F || !dV) return FL_ERR_ARG_NULL;
  ibm_launch_spread(m, ncomp, F, dV, f);
  FL_HIP(hipGetLastError());
  return FL_SUCCESS;
}

extern "C" int fl_ibm_rigid_pose(fl_poisson *h, int64_t L, const double *X0, const double *Y0, const double *Z0, const double centre0[3], const double centre[3], const double rotvec[3], const double velocity[3], const double omega[3],
                                 double *X, double *Y, double *Z, double *Ut)
{
  if (!h || !centre0 || !centre || !rotvec || !velocity || !omega) return FL_ERR_ARG_NULL;
  if (L < 0) return FL_ERR_ARG_OUTOFRANGE;
  if (L == 0) return FL_SUCCESS;
  if (!X0 || !Y0 || !Z0 || (!X != !Y) || (!X != !Z) || (!X && !Ut)) return FL_ERR_ARG_NULL;
  PoseP P;
  for (int a = 0; a < 3; ++a) P.c0[a] = centre0[a], P.c[a] = centre[a], P.v[a] = velocity[a], P.w[a] = omega[a];
  // Rodrigues: R = cos(th) I + sin(th) [k]x + (1 - cos(th)) k k^T, rotvec = th k; formed on the host so that every rank multiplies by the same nine numbers
  const double th = std::sqrt(rotvec[0] * rotvec[0] + rotvec[1] * rotvec[1] + rotvec[2] * rotvec[2]);
  const double k[3] = {th > 0. ? rotvec[0] / th : 0., th > 0. ? rotvec[1] / th : 0., th > 0. ? rotvec[2] / th : 0.};
  const double cs = std::cos(th), sn = std::sin(th);
  const double K[9] = {0., -k[2], k[1], k[2], 0., -k[0], -k[1], k[0], 0.};
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) P.R[3 * a + b] = (a == b ? cs : 0.) + sn * K[3 * a + b] + (1. - cs) * k[a] * k[b];
  FL_HIP(hipSetDevice(h->device));
  hipLaunchKernelGGL(k_ibm_rigid_pose, dim3((unsigned)((L + 255) / 256)), dim3(256), 0, h->stream, L, P, X0, Y0, Z0, X, Y, Z, Ut);
  FL_HIP(hipGetLastError());
  return FL_SUCCESS;
}

// every device array is a DevBuf and frees itself; the one wait covers work that may still read them
extern "C" int fl_ibm_destroy(fl_ibm *m)
{
  if (!m) return FL_SUCCESS;
  if (m->gp) (void)hipStreamSynchronize(m->gp->stream);
  delete m;
  return FL_SUCCESS;
}
