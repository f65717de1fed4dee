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
//   k_ibm_rigid_pose  a rigid body's markers and target velocities from their reference positions (the host mirror's moving body)
//   a scalar held on the markers (fl_ibm_scalar_force, include/fluca_hip_ibm_scalar.h): per pass the bits of interp(1), T - Phi, spread(1)
//   k_ibm_scalar_defect  k_ibm_interp for one field whose lane 0 goes on to q = T - Phi and the running Q (one rank: the defect in the interpolation's launch)
//   k_ibm_scalar_q       one lane per own marker: q and Q from a Phi that is complete (behind k_ibm_collect_U / the all-reduce)
//   k_ibm_spread<1>      the spread's one-component instantiation: one staged value per marker, two accumulators per thread
#include "fl_handle.h"
#include "../../include/fluca_hip_ibm_scalar.h"

namespace fl {

constexpr int TB       = 8;    // tile edge (cells)
constexpr int BIN_CHUNK = 256; // markers staged in LDS per pass

__device__ __forceinline__ double phi_peskin4(double r)
{
  r = fabs(r);
  if (r <= 1.) return (3. - 2. * r + sqrt(1. + 4. * r - 4. * r * r)) / 8.;
  if (r <= 2.) return (5. - 2. * r - sqrt(fmax(-7. + 12. * r - 4. * r * r, 0.))) / 8.;
  return 0.;
}
__device__ __forceinline__ double phi_roma3(double r)
{
  r = fabs(r);
  if (r <= 0.5) return (1. + sqrt(1. - 3. * r * r)) / 3.;
  if (r <= 1.5) return (5. - 3. * r - sqrt(fmax(1. - 3. * (1. - r) * (1. - r), 0.))) / 6.;
  return 0.;
}

struct IbmP {
  int     kind, S;
  int64_t L;
  int     n[3];        // local cells
  int     lo[3];       // global index of local cell 0
  int     ng[3];       // global cells
  int     periodic[3]; // periodic axis of the GLOBAL grid (support indices wrap modulo ng, then ownership is tested)
  double  x0[3], h[3]; // global origin, spacing
  int     nt[3];       // tiles
  int     uniform[3];  // axis with equal spacing: s = (X - x0) / h - 1/2; else the search through xcg
  const double *xcg[3];  // GLOBAL cell centres of a stretched axis, index -1..ng (ghost centres: mirror image / periodic image)
  const double *idx[3];  // LOCAL 1/dx (GridP::idx): the target cell's volume
};

// position -> continuous cell-centre index s along axis d
__device__ __forceinline__ double ibm_index(const IbmP &P, int d, double pos)
{
  if (P.uniform[d]) return (pos - P.x0[d]) / P.h[d] - 0.5;
  // the interval [centre(c), centre(c+1)) that holds the marker, c = -1 .. ng-1 (linear extension beyond the ghost centres)
  const double *xc = P.xcg[d];
  int           lo = -1, hi = P.ng[d] - 1;
  while (lo < hi) {
    const int mid = lo + (hi - lo + 1) / 2;
    if (xc[mid] <= pos) lo = mid;
    else hi = mid - 1;
  }
  return (double)lo + (pos - xc[lo]) / (xc[lo + 1] - xc[lo]);
}
// first support cell (GLOBAL index, may be out of range)
__device__ __forceinline__ int ibm_first(const IbmP &P, double s) { return (P.kind == FL_DELTA_PESKIN4) ? (int)floor(s) - 1 : (int)floor(s + 0.5) - 1; }
// ... as it is stored and handed to support_cell: on a periodic axis taken modulo ng, so that a position any number of periods beyond either end
// counts as its image in the box (the rule of k_ibm_route's ownership test and of the oracle), and first + a < ng + S: the single wrap of
// support_cell and of k_ibm_spread's staging step is a full one.  The weights are formed from the unwrapped index.
__device__ __forceinline__ int ibm_wrap_first(const IbmP &P, int d, int i)
{
  if (!P.periodic[d]) return i;
  i %= P.ng[d];
  return i < 0 ? i + P.ng[d] : i;
}

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

// LOCAL cell index of support entry a, or -1 when that cell is not owned by this rank.  Every rank sees every marker whose
// support touches its block (replicated markers: all of them; owner-rank markers: its own and the ghost copies); a support
// that straddles a block face is simply shared out between the two owners, and a support that crosses a periodic boundary
// wraps in GLOBAL index space first (once: i0 comes from ibm_wrap_first).
__device__ __forceinline__ int support_cell(const IbmP &P, int d, int i0, int a)
{
  int c = i0 + a;
  if (P.periodic[d]) {
    if (c < 0) c += P.ng[d];
    else if (c >= P.ng[d]) c -= P.ng[d];
  }
  c -= P.lo[d];
  return (c < 0 || c >= P.n[d]) ? -1 : c;
}

// the distinct tiles the support touches along each axis: at most 3 (S=4 over 8-cell tiles gives <= 2, a wrap adds one)
__device__ __forceinline__ int support_tiles(const IbmP &P, int d, int i0, int t[4])
{
  int nt = 0;
  for (int a = 0; a < P.S; ++a) {
    const int c = support_cell(P, d, i0, a);
    if (c < 0) continue;
    const int tt = c / TB;
    bool      dup = false;
    for (int b = 0; b < nt; ++b) dup |= (t[b] == tt);
    if (!dup) t[nt++] = tt;
  }
  return nt;
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

// ---- owner-rank markers ---------------------------------------------------------------------------------------------------------
// Neighbour offsets o in {-1,0,1}^3 are numbered code = (oz+1)*9 + (oy+1)*3 + (ox+1); 13 is the block itself, 26 - code the opposite offset.
struct RouteP {
  int peer_lo[3], peer_hi[3];  // a rank sits behind the low / high end of the block along this axis (not a wall, not an axis one rank holds alone)
};

// the cell that decides the owner along axis d (GLOBAL index), s = the marker's continuous cell-centre index: k_ibm_route and k_ibm_dest share it
__device__ __forceinline__ int ibm_owner_cell(const IbmP &P, int d, double s)
{
  int c = (int)floor(s + 0.5);
  if (P.periodic[d]) {
    c %= P.ng[d];
    if (c < 0) c += P.ng[d];
  } else c = min(max(c, 0), P.ng[d] - 1);
  return c;
}

// mask[l] = the set of offsets (bit = code) whose blocks the support of own marker l reaches, or -1 when the marker does not belong to this
// rank.  THE OWNERSHIP RULE: the marker belongs to the block that holds the cell floor(s_d + 1/2) on every axis, the index wrapped on a periodic
// axis and clamped to [0, ng-1] otherwise -- global quantities only, so every marker has exactly one owner.  That cell lies inside the support of
// either delta function, so along an axis the support leaves a block of >= 4 cells through one end at most: below, if its first entries are not
// this rank's (support_cell < 0), above, if its last ones are not.
__global__ void k_ibm_route(IbmP P, RouteP R, const double *__restrict__ X, const double *__restrict__ Y, const double *__restrict__ Z, int *__restrict__ mask)
{
  const int64_t l = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (l >= P.L) return;
  const double pos[3] = {X[l], Y[l], Z[l]};
  bool         mine = true, dn[3], up[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    const double s = ibm_index(P, d, pos[d]);
    const int    c = ibm_owner_cell(P, d, s);
    mine = mine && c >= P.lo[d] && c < P.lo[d] + P.n[d];
    const int i     = ibm_wrap_first(P, d, ibm_first(P, s));
    int       first = -1, last = -1;
    for (int a = 0; a < P.S; ++a)
      if (support_cell(P, d, i, a) >= 0) {
        if (first < 0) first = a;
        last = a;
      }
    dn[d] = first > 0 && R.peer_lo[d];
    up[d] = last >= 0 && last < P.S - 1 && R.peer_hi[d];
  }
  int bits = 0;
  for (int code = 0; code < 27; ++code) {
    if (code == 13) continue;
    const int o[3] = {code % 3 - 1, (code / 3) % 3 - 1, code / 9 - 1};
    bool      hit  = true;
#pragma unroll
    for (int d = 0; d < 3; ++d) hit = hit && (o[d] == 0 || (o[d] < 0 ? dn[d] : up[d]));
    if (hit) bits |= 1 << code;
  }
  mask[l] = mine ? bits : -1;
}

// Messages hold one record per copy, the copies of an offset next to each other (the send list is grouped by ascending offset code, the
// ghosts are stored in that order too): a message is a contiguous piece of the buffer and no kernel needs to know where one ends.
// positions: (X, Y, Z, gid) of the copies through the send list
__global__ void k_ibm_pack_pos(int ncopy, const int *__restrict__ sendlist, const double *__restrict__ X, const double *__restrict__ Y, const double *__restrict__ Z, const int64_t *__restrict__ gid, double *__restrict__ buf)
{
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= ncopy) return;
  const int l    = sendlist[j];
  buf[4 * j + 0] = X[l];
  buf[4 * j + 1] = Y[l];
  buf[4 * j + 2] = Z[l];
  buf[4 * j + 3] = gid ? (double)gid[l] : 0.;  // marker numbers stay below 2^27: exact
}
// ... and into the marker arrays behind the Lo own markers
__global__ void k_ibm_unpack_pos(int nghost, int64_t Lo, const double *__restrict__ buf, double *__restrict__ X, double *__restrict__ Y, double *__restrict__ Z, int64_t *__restrict__ gid)
{
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= nghost) return;
  X[Lo + g] = buf[4 * g + 0];
  Y[Lo + g] = buf[4 * g + 1];
  Z[Lo + g] = buf[4 * g + 2];
  if (gid) gid[Lo + g] = (int64_t)buf[4 * g + 3];
}
// interp: the ghosts' partial sums (Ui: ncomp x Lt, own markers first) as records of ncomp
__global__ void k_ibm_pack_U(int nghost, int64_t Lo, int64_t Lt, int ncomp, const double *__restrict__ Ui, double *__restrict__ buf)
{
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= nghost) return;
  for (int c = 0; c < ncomp; ++c) buf[(int64_t)g * ncomp + c] = Ui[(int64_t)c * Lt + Lo + g];
}
// interp: U of own marker l = its own partial sum + those of its copies cl[cs[l] .. cs[l+1]) in ascending copy number (= offset code)
__global__ void k_ibm_collect_U(int64_t Lo, int64_t Lt, int ncomp, const double *__restrict__ Ui, const int *__restrict__ cs, const int *__restrict__ cl, const double *__restrict__ buf, double *__restrict__ U)
{
  const int64_t l = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (l >= Lo) return;
  const int beg = cs[l], end = cs[l + 1];
  for (int c = 0; c < ncomp; ++c) {
    double v = Ui[(int64_t)c * Lt + l];
    for (int j = beg; j < end; ++j) v += buf[(int64_t)cl[j] * ncomp + c];
    U[(int64_t)c * Lo + l] = v;
  }
}
// spread: (F_0 .. F_ncomp-1, dV) of the copies through the send list
__global__ void k_ibm_pack_F(int ncopy, int64_t Lo, int ncomp, const int *__restrict__ sendlist, const double *__restrict__ F, const double *__restrict__ dV, double *__restrict__ buf)
{
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= ncopy) return;
  const int l = sendlist[j];
  for (int c = 0; c < ncomp; ++c) buf[(int64_t)j * (ncomp + 1) + c] = F[(int64_t)c * Lo + l];
  buf[(int64_t)j * (ncomp + 1) + ncomp] = dV[l];
}
// spread: F / dV of own + ghost markers in the layout k_ibm_spread reads (stride Lt): the caller's for the own ones, the records received for the ghosts
__global__ void k_ibm_stage_F(int64_t Lo, int64_t Lt, int ncomp, const double *__restrict__ F, const double *__restrict__ dV, const double *__restrict__ buf, double *__restrict__ Fi, double *__restrict__ dVi)
{
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= Lt) return;
  if (t < Lo) {
    for (int c = 0; c < ncomp; ++c) Fi[(int64_t)c * Lt + t] = F[(int64_t)c * Lo + t];
    dVi[t] = dV[t];
  } else {
    const int64_t g = t - Lo;
    for (int c = 0; c < ncomp; ++c) Fi[(int64_t)c * Lt + t] = buf[g * (ncomp + 1) + c];
    dVi[t] = buf[g * (ncomp + 1) + ncomp];
  }
}

// ---- owner-rank markers: migration (fl_ibm_migrate) ------------------------------------------------------------------------------------
// Every record and every staging array below is made of doubles: position, the marker number (< 2^27: exact) and up to 8 attributes.
constexpr int MIG_NCNT = 32;  // cnt[0..26] markers per destination offset (13: stay), cnt[27] out of reach, cnt[28] numbers not ascending, cnt[29] spare

struct DestP {
  int peer_lo[3], peer_hi[3];      // RouteP's
  int lo_beg[3], lo_end[3];        // GLOBAL cells [beg, end) of the block behind the low end of this one along the axis (the periodic wrap included)
  int hi_beg[3], hi_end[3];        // ... behind the high end
};

// dest[l] = the offset code of the block that owns own marker l at its NEW position: 13 it stays, -1 neither this block nor a neighbour holds the cell.
// Where the low and the high neighbour are one rank (two ranks on a periodic axis) the low one is taken.  cnt: per code, formed per wave (ballot and
// popcount, the first lane of every code adds once); blockstay[b] = stayers among the block's 256 markers, the input of the compaction's scan.
__global__ void __launch_bounds__(256) k_ibm_dest(IbmP P, DestP D, const double *__restrict__ X, const double *__restrict__ Y, const double *__restrict__ Z, const int64_t *__restrict__ gid, int *__restrict__ dest, int *__restrict__ cnt,
                                                  int *__restrict__ blockstay)
{
  __shared__ int wstay[4];
  const int64_t  l     = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int      lane  = threadIdx.x & 63;
  const bool     valid = l < P.L;
  int            code  = -1;
  bool           unsorted = false;
  if (valid) {
    const double pos[3] = {X[l], Y[l], Z[l]};
    int          o[3];
    bool         reach = true;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      const int c = ibm_owner_cell(P, d, ibm_index(P, d, pos[d]));
      if (c >= P.lo[d] && c < P.lo[d] + P.n[d]) o[d] = 0;
      else if (D.peer_lo[d] && c >= D.lo_beg[d] && c < D.lo_end[d]) o[d] = -1;
      else if (D.peer_hi[d] && c >= D.hi_beg[d] && c < D.hi_end[d]) o[d] = 1;
      else o[d] = 0, reach = false;
    }
    code = reach ? (o[2] + 1) * 9 + (o[1] + 1) * 3 + (o[0] + 1) : -1;
    dest[l]  = code;
    unsorted = l > 0 && gid[l - 1] >= gid[l];
  }
  unsigned long long todo = __ballot(valid);
  while (todo) {  // wave-uniform: one round per distinct code in the wave
    const int                leader = __ffsll((long long)todo) - 1;
    const int                c      = __shfl(code, leader, 64);
    const unsigned long long same   = __ballot(valid && code == c);
    if (lane == leader) atomicAdd(&cnt[c < 0 ? 27 : c], __popcll(same));
    todo &= ~same;
  }
  if (__ballot(unsorted) != 0ull && lane == 0) atomicOr(&cnt[28], 1);
  const unsigned long long stay = __ballot(valid && code == 13);
  if (lane == 0) wstay[threadIdx.x >> 6] = __popcll(stay);
  __syncthreads();
  if (threadIdx.x == 0) blockstay[blockIdx.x] = wstay[0] + wstay[1] + wstay[2] + wstay[3];
}

// Stayers keep their order: index = blockoff[block] (k_ibm_scan over blockstay) + the stayers of the waves before + those of the lanes before
// (ballot).  stay[f*Ls + i], f = X, Y, Z, number, attributes.  Leavers become records of per = 4 + nattr doubles in buf, grouped by code through
// leaveoff[code] and one cursor per code (the order inside a group is free: the receiver sorts by number).
__global__ void __launch_bounds__(256) k_ibm_split(int64_t Lo, int64_t Ls, int nattr, const int *__restrict__ dest, const int *__restrict__ blockoff, const int *__restrict__ leaveoff, int *__restrict__ cursor, const double *__restrict__ X,
                                                   const double *__restrict__ Y, const double *__restrict__ Z, const int64_t *__restrict__ gid, const double *__restrict__ attr, double *__restrict__ stay, double *__restrict__ buf)
{
  __shared__ int wstay[4];
  const int64_t  l     = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int      lane  = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int      code  = l < Lo ? dest[l] : -1;
  const unsigned long long stays = __ballot(code == 13);
  if (lane == 0) wstay[wave] = __popcll(stays);
  __syncthreads();
  if (l >= Lo) return;
  const double g = (double)gid[l];
  if (code == 13) {
    int64_t i = blockoff[blockIdx.x] + __popcll(stays & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; ++w) i += wstay[w];
    if (i >= Ls) return;  // cannot happen: the counts come from the same dest[]
    stay[i]          = X[l];
    stay[Ls + i]     = Y[l];
    stay[2 * Ls + i] = Z[l];
    stay[3 * Ls + i] = g;
    for (int a = 0; a < nattr; ++a) stay[(4 + a) * Ls + i] = attr[(int64_t)a * Lo + l];
  } else if (code >= 0) {
    const int     per = 4 + nattr;
    const int64_t j   = leaveoff[code] + atomicAdd(&cursor[code], 1);
    if (j >= leaveoff[code + 1]) return;  // cannot happen either
    buf[per * j + 0] = X[l];
    buf[per * j + 1] = Y[l];
    buf[per * j + 2] = Z[l];
    buf[per * j + 3] = g;
    for (int a = 0; a < nattr; ++a) buf[per * j + 4 + a] = attr[(int64_t)a * Lo + l];
  }
}

// Arrivals (A records of per doubles, as received) -> arr[f*A + r], r = the rank of the record's number among all arrivals (ties, which distinct
// numbers do not make, by record index).  Rank by counting as k_ibm_sort_bins does for a bin, the numbers tiled through LDS: O(A^2).
__global__ void __launch_bounds__(256) k_ibm_rank_arrivals(int A, int per, const double *__restrict__ buf, double *__restrict__ arr)
{
  __shared__ double tile[256];
  const int    e  = blockIdx.x * 256 + threadIdx.x;
  const double ge = e < A ? buf[(int64_t)per * e + 3] : 0.;
  int          rank = 0;
  for (int base = 0; base < A; base += 256) {
    __syncthreads();
    tile[threadIdx.x] = base + (int)threadIdx.x < A ? buf[(int64_t)per * (base + threadIdx.x) + 3] : 0.;
    __syncthreads();
    const int n = min(256, A - base);
    for (int o = 0; o < n; ++o) rank += (tile[o] < ge) || (tile[o] == ge && base + o < e);
  }
  if (e >= A) return;
  for (int f = 0; f < per; ++f) arr[(int64_t)f * A + rank] = buf[(int64_t)per * e + f];
}

// number of entries of the ascending key[0..n) below v (or, with_equal, not above it)
__device__ __forceinline__ int64_t ibm_count_below(const double *__restrict__ key, int64_t n, double v, bool with_equal)
{
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo) / 2;
    if (key[mid] < v || (with_equal && key[mid] == v)) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// Stayers and sorted arrivals, both ascending in the number, into one ascending list without a sort: a stayer moves up by the arrivals below it, an
// arrival by the stayers below it (ties would go stayer first, so the indices are a permutation whatever the numbers are).
// pos[f*Ln + i] f = X, Y, Z; gid[i]; attr[a*Ln + i]
__global__ void k_ibm_merge(int64_t Ls, int64_t A, int nattr, const double *__restrict__ stay, const double *__restrict__ arr, double *__restrict__ pos, int64_t *__restrict__ gid, double *__restrict__ attr)
{
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, Ln = Ls + A;
  if (t >= Ln) return;
  const bool    st  = t < Ls;
  const int64_t i   = st ? t : t - Ls, n = st ? Ls : A;
  const double *src = st ? stay : arr;
  const double  g   = src[3 * n + i];
  const int64_t to  = i + (st ? ibm_count_below(arr + 3 * A, A, g, false) : ibm_count_below(stay + 3 * Ls, Ls, g, true));
  pos[to]          = src[i];
  pos[Ln + to]     = src[n + i];
  pos[2 * Ln + to] = src[2 * n + i];
  gid[to]          = (int64_t)g;
  for (int a = 0; a < nattr; ++a) attr[(int64_t)a * Ln + to] = src[(4 + a) * n + i];
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

// ---- force and torque on each body (fl_ibm_force) -----------------------------------------------------------------------------------------
// force_b = sum_l F_l dV_l, torque_b = sum_l (r_l x F_l) dV_l over the markers of body b, r_l = X_l - about_b (minimum image on a periodic axis),
// as a sum whose bits do not depend on the order of the markers or on how they are shared out between ranks:
//   terms    every product, difference and quotient rounded once, never contracted into a fused multiply-add (force_terms)
//   max pass amax = max |t| over a group (the 3 nbody force sums; the 3 nbody torque sums), a non-finite term counts as +inf; E: amax < 2^E
//   split    t = a 2^(E-30) + b 2^(E-60) + tail, a = rint(t / 2^(E-30)), b = rint((t - a 2^(E-30)) / 2^(E-60)): integers of at most 31 bits, so
//            that sums of fewer than 2^22 of them are exact in a double in ANY order; |tail| <= 2^(E-61)
//   result   (sum a) 2^(E-30) + (sum b) 2^(E-60), the one rounding of the whole sum, formed on the host (force_combine)
// Where 2^(E-60) would be subnormal (E < -900) the group is scaled by 2^FORCE_UP, an exact operation, and the result scaled back.
constexpr int FORCE_MAXBLK = 64;   // blocks of 256 per pass: the grid-stride loop covers the rest, no second round of blocks
constexpr int FORCE_MAXBODY = 64;
constexpr int FORCE_UP = 200;
// workspace (doubles): header { amax force, amax torque, bad body id, spare }, the 12 nbody sums, about, the max pass' block partials, the slabs
constexpr int FW_SUMS = 4, FW_ABOUT = FW_SUMS + 12 * FORCE_MAXBODY, FW_PART = FW_ABOUT + 3 * FORCE_MAXBODY, FW_SLAB = FW_PART + 4 * FORCE_MAXBLK,
              FW_END = FW_SLAB + FORCE_MAXBLK * 12 * FORCE_MAXBODY;

struct ForceP {
  int64_t L;
  int     nbody;
  int     periodic[3];
  double  per[3];    // period of a periodic axis: xf[n] - xf[0]
  double  about[3];  // one body (no body array): the reference point, so that nothing is indexed
};

// the six terms of marker l: F_c dV and ((r x F)_c) dV
__device__ __forceinline__ void force_terms(const ForceP &Q, const double *__restrict__ X, const double *__restrict__ Y, const double *__restrict__ Z, const double *__restrict__ F, const double *__restrict__ dV, int64_t l,
                                            const double *ab, double t[6])
{
#pragma clang fp contract(off)
  const double pos[3] = {X[l], Y[l], Z[l]};
  const double f[3]   = {F[l], F[Q.L + l], F[2 * Q.L + l]};
  const double dv     = dV[l];
  double       r[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    r[d] = pos[d] - ab[d];
    if (Q.periodic[d]) {
      const double q = rint(r[d] / Q.per[d]);
      const double s = Q.per[d] * q;
      r[d]           = r[d] - s;
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int    c1 = (c + 1) % 3, c2 = (c + 2) % 3;
    const double p1 = r[c1] * f[c2], p2 = r[c2] * f[c1];
    const double cr = p1 - p2;
    t[c]            = f[c] * dv;
    t[3 + c]        = cr * dv;
  }
}
__device__ __forceinline__ double force_mag(double t)
{
  const double a = fabs(t);
  return a <= 1.7976931348623157e308 ? a : __builtin_inf();  // NaN fails the comparison too: fmax would drop it
}
// amax -> the exponents of the split: a = rint(t 2^sa), rem = t 2^up - a 2^ea, b = rint(rem 2^sb); live: the group has a finite, non-zero term
struct ForceSplit {
  int live, up, sa, ea, sb;
};
__host__ __device__ inline ForceSplit force_split(double amax)
{
  ForceSplit s = {0, 0, 0, 0, 0};
  if (!(amax > 0.) || !(amax <= 1.7976931348623157e308)) return s;
  const int E = ilogb(amax) + 1;  // amax < 2^E
  s.live      = 1;
  s.up        = E < -900 ? FORCE_UP : 0;
  s.sa        = 30 - E;
  s.ea        = E + s.up - 30;
  s.sb        = 60 - E - s.up;
  return s;
}
// the value of a group's sum from its two exact integer sums
static double force_combine(double amax, double A, double B)
{
  if (!(amax <= 1.7976931348623157e308)) return std::nan("");
  const ForceSplit s = force_split(amax);
  if (!s.live) return 0.;
  return std::ldexp(std::ldexp(A, s.ea) + std::ldexp(B, s.ea - 30), -s.up);
}

// Hand-off of block partials to the last-arriving block, as k_cg_Bq's (fl_kernels.hip, fused_fin): agent-scope (write-through) stores, every
// storing wave drains them, the block meets, one lane draws a ticket; the block that draws the last one reads every partial with agent-scope
// loads.  The counter is zeroed by the caller before every launch.
__device__ __forceinline__ bool force_last_block(unsigned *counter, int *flag)
{
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned t = __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    *flag            = (t == gridDim.x - 1u);
  }
  __syncthreads();
  return *flag != 0;
}

// max pass: ws[0] / ws[1] = max |t| of the force / torque terms (+inf: a non-finite term), ws[2] = 1 if a body id lies outside 0..nbody-1
template <bool BODY>
__global__ void __launch_bounds__(256) k_ibm_force_max(ForceP Q, const double *__restrict__ X, const double *__restrict__ Y, const double *__restrict__ Z, const double *__restrict__ F, const double *__restrict__ dV,
                                                       const int32_t *__restrict__ body, double *__restrict__ ws, unsigned *__restrict__ counter)
{
  __shared__ double red[4][3];
  __shared__ int    flag;
  const int         lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double            m[3] = {0., 0., 0.};
  for (int64_t l = (int64_t)blockIdx.x * 256 + threadIdx.x; l < Q.L; l += (int64_t)gridDim.x * 256) {
    double        t[6];
    const double *ab = Q.about;
    if (BODY) {
      const int b = body[l];
      if (b < 0 || b >= Q.nbody) {
        m[2] = 1.;
        continue;
      }
      ab = ws + FW_ABOUT + 3 * b;
    }
    force_terms(Q, X, Y, Z, F, dV, l, ab, t);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      m[0] = fmax(m[0], force_mag(t[c]));
      m[1] = fmax(m[1], force_mag(t[3 + c]));
    }
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m[a] = fmax(m[a], __shfl_xor(m[a], o, 64));
    if (lane == 0) red[wave][a] = m[a];
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    const double v = fmax(fmax(red[0][threadIdx.x], red[1][threadIdx.x]), fmax(red[2][threadIdx.x], red[3][threadIdx.x]));
    __hip_atomic_store(&ws[FW_PART + 4 * blockIdx.x + threadIdx.x], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if (!force_last_block(counter, &flag)) return;
  if (wave == 0) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      double v = lane < (int)gridDim.x ? __hip_atomic_load(&ws[FW_PART + 4 * lane + a], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
      if (lane == 0) ws[a] = v;
    }
  }
}

// split-and-sum pass: ws[FW_SUMS + (b*6 + term)*2 + part] = the sum over body b's markers of the integers a (part 0) and b (part 1) of term
// 0..2 (force) / 3..5 (torque).  Every partial sum is an exact integer below 2^53, so wave shuffles, LDS atomics and the block order are all free.
template <bool BODY>
__global__ void __launch_bounds__(256) k_ibm_force_sum(ForceP Q, const double *__restrict__ X, const double *__restrict__ Y, const double *__restrict__ Z, const double *__restrict__ F, const double *__restrict__ dV,
                                                       const int32_t *__restrict__ body, double *__restrict__ ws, unsigned *__restrict__ counter)
{
  __shared__ double acc[BODY ? 12 * FORCE_MAXBODY : 4 * 12];
  __shared__ int    flag;
  const int         lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int         n    = 12 * Q.nbody;
  const ForceSplit  sp[2] = {force_split(ws[0]), force_split(ws[1])};
  double            s[12];
#pragma unroll
  for (int j = 0; j < 12; ++j) s[j] = 0.;
  if (BODY) {
    for (int j = threadIdx.x; j < n; j += 256) acc[j] = 0.;
    __syncthreads();
  }
  for (int64_t l = (int64_t)blockIdx.x * 256 + threadIdx.x; l < Q.L; l += (int64_t)gridDim.x * 256) {
    double        t[6];
    const double *ab = Q.about;
    int           b  = 0;
    if (BODY) {
      b = body[l];
      if (b < 0 || b >= Q.nbody) continue;  // the max pass has flagged it: the call fails and the sums are not used
      ab = ws + FW_ABOUT + 3 * b;
    }
    force_terms(Q, X, Y, Z, F, dV, l, ab, t);
#pragma unroll
    for (int c = 0; c < 6; ++c) {
      const ForceSplit &g = sp[c / 3];
      double            ia = 0., ib = 0.;
      if (g.live) {
        ia               = rint(ldexp(t[c], g.sa));
        const double rem = ldexp(t[c], g.up) - ldexp(ia, g.ea);  // exact: the bits of t below 2^(E-30)
        ib               = rint(ldexp(rem, g.sb));
      }
      if (BODY) {
        if (ia != 0.) atomicAdd(&acc[b * 12 + 2 * c], ia);
        if (ib != 0.) atomicAdd(&acc[b * 12 + 2 * c + 1], ib);
      } else {
        s[2 * c] += ia;
        s[2 * c + 1] += ib;
      }
    }
  }
  if (!BODY) {
#pragma unroll
    for (int j = 0; j < 12; ++j) {
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) s[j] += __shfl_xor(s[j], o, 64);
      if (lane == 0) acc[wave * 12 + j] = s[j];
    }
  }
  __syncthreads();
  for (int j = threadIdx.x; j < n; j += 256) {
    const double v = BODY ? acc[j] : (acc[j] + acc[12 + j]) + (acc[24 + j] + acc[36 + j]);
    __hip_atomic_store(&ws[FW_SLAB + (int64_t)blockIdx.x * n + j], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if (!force_last_block(counter, &flag)) return;
  for (int j = threadIdx.x; j < n; j += 256) {
    double v = 0.;
    for (int blk = 0; blk < (int)gridDim.x; ++blk) v += __hip_atomic_load(&ws[FW_SLAB + (int64_t)blk * n + j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    ws[FW_SUMS + j] = v;
  }
}

// ---- Dirichlet forcing of one scalar on the markers (fl_ibm_scalar_force) ---------------------------------------------------------------------
// One pass: Phi = interp(phi), q = T - Phi, Q (+)= q, phi += spread(q, dV) -- the bits of fl_ibm_interp(1), fl_vec_lincomb(-1 Phi + 1 T) and
// fl_ibm_spread(1) one after the other.  The difference is rounded once either way: a product with -1 or 1 is exact.
struct ScalarTarget {
  double value[FORCE_MAXBODY];  // the per-body table, passed by value: the caller's host array is read before the call returns
};
__device__ __forceinline__ double scalar_target(const double *__restrict__ target, const int32_t *__restrict__ body, const ScalarTarget &V, int64_t l)
{
  return target ? target[l] : V.value[body ? body[l] : 0];  // ids are the caller's promise: nothing is clamped or checked here
}

// k_ibm_interp for one field -- its lanes, its weights, its fixed-order reduction -- and lane 0 goes on to the defect: q[l] = T_l - Phi_l,
// Q[l] = q[l] (first pass) or Q[l] + q[l].  One rank only: where partial sums of other ranks belong to Phi, k_ibm_scalar_q forms q behind them.
__global__ void __launch_bounds__(256) k_ibm_scalar_defect(IbmP P, const int *__restrict__ i0, const double *__restrict__ w, const double *__restrict__ phi, const double *__restrict__ target, const int32_t *__restrict__ body,
                                                           ScalarTarget V, int first, double *__restrict__ q, double *__restrict__ Q)
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
  double v = cell >= 0 ? wt * phi[cell] : 0.;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  if (lane == 0) {
    const double d = scalar_target(target, body, V, l) - v;
    q[l]           = d;
    if (Q) Q[l] = first ? d : Q[l] + d;
  }
}

// the defect of own marker l from a Phi that is complete (behind k_ibm_collect_U on an owned set, behind the all-reduce on a replicated one)
__global__ void k_ibm_scalar_q(int64_t L, const double *__restrict__ Phi, const double *__restrict__ target, const int32_t *__restrict__ body, ScalarTarget V, int first, double *__restrict__ q, double *__restrict__ Q)
{
  const int64_t l = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (l >= L) return;
  const double d = scalar_target(target, body, V, l) - Phi[l];
  q[l]           = d;
  if (Q) Q[l] = first ? d : Q[l] + d;
}

}  // namespace fl

using namespace fl;

struct fl_ibm {
  fl_poisson *gp = nullptr;
  IbmP        P;
  double     *X = nullptr, *Y = nullptr, *Z = nullptr, *w = nullptr;
  int        *i0 = nullptr, *cnt = nullptr, *off = nullptr, *list = nullptr, *scratch = nullptr, *active = nullptr, *nact_dev = nullptr;
  int         ntiles = 0, listcap = 0, nactive = 0;
  int64_t     cap = -1;                               // markers the per-marker arrays above hold
  double     *xcg[3] = {nullptr, nullptr, nullptr};  // device copies of the extended global centre arrays (stretched axes only)
  // owner-rank markers (fl_ibm_create_owned): P.L = Lo + Lg, own markers first, then the ghosts grouped by ascending offset code
  bool        owned = false, has_gid = false;
  int64_t     Lo = 0, Lg = 0;                         // own markers, ghost markers held
  int         ncopy = 0;                              // copies of own markers held by other ranks
  RouteP      R;
  int         peer[27], scnt[27], soff[27], gcnt[27], goff[27];  // per offset code: rank behind it (-1 none), copies sent / ghosts held and where they start
  int64_t    *gid_own = nullptr, *gid = nullptr;      // the caller's marker numbers: of the own markers (kept for update), of own + ghost (sort key)
  int        *mask = nullptr, *sendlist = nullptr, *cstart = nullptr, *clist = nullptr;
  int64_t     maskcap = 0;
  double     *sbuf = nullptr, *rbuf = nullptr, *Ui = nullptr, *Fi = nullptr, *cbuf = nullptr;  // message records out / in, U and (F, dV) of own + ghost, counts
  int64_t     sbufcap = 0, rbufcap = 0, Uicap = 0, Ficap = 0;
  // migration (fl_ibm_migrate): neighbours' cell ranges (exchanged once), staging buffers, the attributes of the last call
  bool        nbr_known = false;
  DestP       D;
  int64_t     gidowncap = 0;
  int        *dest = nullptr, *bstay = nullptr, *boff = nullptr, *mcnt = nullptr;  // per marker; per block of 256 (count, offset); MIG_NCNT counts + 28 offsets + 27 cursors
  int64_t    *gidtmp = nullptr;
  double     *stay = nullptr, *arr = nullptr, *mpos = nullptr, *attr = nullptr, *attrtmp = nullptr, *nbuf = nullptr;
  int64_t     destcap = 0, bstaycap = 0, boffcap = 0, gidtmpcap = 0, staycap = 0, arrcap = 0, mposcap = 0, attrcap = 0, attrtmpcap = 0;
  int         nattr = 0;
  // fl_ibm_force: workspace (FW_END doubles) and the two arrival counters (16 bytes, zeroed before every call)
  double     *fws = nullptr;
  unsigned   *ftick = nullptr;
  // fl_ibm_scalar_force / fl_ibm_scalar_rate: q and the complete Phi of a pass (one value per marker of the set), (Q, 0, 0) for the rate's sum
  double     *sq = nullptr, *sphi = nullptr, *sf3 = nullptr;
  int64_t     sqcap = 0, sphicap = 0, sf3cap = 0;
};

static int ibm_rebin(fl_ibm *m)
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
  hipLaunchKernelGGL(k_ibm_scan, dim3(1), dim3(256), 0, s, m->cnt, m->off, m->ntiles);
  FL_HIP(hipMemsetAsync(m->cnt, 0, sizeof(int) * (m->ntiles + 1), s));
  hipLaunchKernelGGL(k_ibm_bin, dim3(nb), dim3(256), 0, s, P, m->i0, m->cnt, m->off, m->list, 1);
  FL_HIP(hipMemsetAsync(m->nact_dev, 0, sizeof(int), s));
  hipLaunchKernelGGL(k_ibm_active, dim3((m->ntiles + 255) / 256), dim3(256), 0, s, m->off, m->ntiles, m->active, m->nact_dev);
  FL_HIP(hipMemcpyAsync(&m->nactive, m->nact_dev, sizeof(int), hipMemcpyDeviceToHost, s));
  FL_HIP(hipStreamSynchronize(s));  // set-up time only (create / marker update), never inside interp / spread
  // sort only the non-empty bins (ascending marker id -> run-independent accumulation order)
  if (m->nactive > 0) hipLaunchKernelGGL(k_ibm_sort_bins, dim3(m->nactive), dim3(256), 0, s, m->off, m->list, m->scratch, m->active, (const int64_t *)(m->has_gid ? m->gid : nullptr));
  FL_HIP(hipGetLastError());
  return 0;
}

static void ibm_free(fl_poisson *h, void *pp)
{
  void **p = (void **)pp;
  if (*p) {
    (void)hipStreamSynchronize(h->stream);
    (void)hipFree(*p);
  }
  *p = nullptr;
}

// the per-marker arrays for L markers (own + ghost of an owner-rank set: the number changes with every update)
static int ibm_alloc_markers(fl_ibm *m, int64_t L)
{
  fl_poisson *h = m->gp;
  if (L <= m->cap) return 0;
  for (void *p : {(void *)&m->X, (void *)&m->Y, (void *)&m->Z, (void *)&m->w, (void *)&m->i0, (void *)&m->list, (void *)&m->scratch, (void *)&m->gid}) ibm_free(h, p);
  m->listcap = (int)std::min<int64_t>(L * 27, (int64_t)1 << 30);
  int rc     = 0;
  rc |= fl_dev_alloc(h, (void **)&m->X, sizeof(double) * L, false);
  rc |= fl_dev_alloc(h, (void **)&m->Y, sizeof(double) * L, false);
  rc |= fl_dev_alloc(h, (void **)&m->Z, sizeof(double) * L, false);
  rc |= fl_dev_alloc(h, (void **)&m->w, sizeof(double) * 12 * L, false);
  rc |= fl_dev_alloc(h, (void **)&m->i0, sizeof(int) * 3 * L, false);
  rc |= fl_dev_alloc(h, (void **)&m->list, sizeof(int) * m->listcap, true);
  rc |= fl_dev_alloc(h, (void **)&m->scratch, sizeof(int) * m->listcap, true);
  if (m->owned) rc |= fl_dev_alloc(h, (void **)&m->gid, sizeof(int64_t) * L, true);
  if (rc) return FL_ERR_MEM;
  m->cap = L;
  return 0;
}

// a buffer of at least `need` elements (grown, never shrunk; the old contents are not kept)
template <class T>
static int ibm_reserve(fl_poisson *h, T **p, int64_t *cap, int64_t need)
{
  if (*p && need <= *cap) return 0;
  ibm_free(h, p);
  need = std::max<int64_t>(need + need / 4, 64);
  if (fl_dev_alloc(h, (void **)p, sizeof(T) * (size_t)need, true)) return FL_ERR_MEM;
  *cap = need;
  return 0;
}

// grid, block and delta function of a marker set; xcg[d] receives the device copy of a stretched axis' centres (the caller frees it)
static int ibm_geometry(fl_poisson *h, int kind, IbmP &P, double *xcg[3])
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
      if (hipMalloc((void **)&xcg[d], sizeof(double) * xc.size()) != hipSuccess || hipMemcpy(xcg[d], xc.data(), sizeof(double) * xc.size(), hipMemcpyHostToDevice) != hipSuccess) return FL_ERR_GPU;
      P.xcg[d] = xcg[d] + 1;
    }
    if (P.periodic[d] && P.ng[d] < 2 * P.S) return FL_ERR_ARG_OUTOFRANGE;
    P.nt[d] = (P.n[d] + TB - 1) / TB;
  }
  return 0;
}

static int ibm_new(fl_poisson *h, int kind, bool owned, fl_ibm **out)
{
  fl_ibm *m = new fl_ibm();
  m->gp     = h;
  m->owned  = owned;
  int rc    = ibm_geometry(h, kind, m->P, m->xcg);
  if (!rc) {
    const IbmP &P = m->P;
    m->ntiles     = P.nt[0] * P.nt[1] * P.nt[2];
    int bad       = 0;
    bad |= fl_dev_alloc(h, (void **)&m->cnt, sizeof(int) * (m->ntiles + 1), true);
    bad |= fl_dev_alloc(h, (void **)&m->off, sizeof(int) * (m->ntiles + 1), true);
    bad |= fl_dev_alloc(h, (void **)&m->active, sizeof(int) * m->ntiles, true);
    bad |= fl_dev_alloc(h, (void **)&m->nact_dev, sizeof(int), true);
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
  if (kind != FL_DELTA_PESKIN4 && kind != FL_DELTA_ROMA3) return FL_ERR_ARG_OUTOFRANGE;
  if (L < 1 || L > (int64_t)1 << 27) return FL_ERR_ARG_OUTOFRANGE;
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

// ---- owner-rank markers: routing (set-up time: host waits as in ibm_rebin) -----------------------------------------------------------

static bool ibm_split(const fl_poisson *h) { return h->dec.ranks[0] * h->dec.ranks[1] * h->dec.ranks[2] > 1; }

// sum of n <= 8 flags over the ranks: every rank takes the same way out of a collective call
static int ibm_vote(fl_poisson *h, double *v, int n)
{
  if (!ibm_split(h)) return 0;
  if (h->comm.kind == Comm::NONE) return FL_ERR_ARG_WRONGSTATE;
  return fl_poisson_allreduce_sum(h, v, n);
}

// the masks of k_ibm_route for L markers at (X, Y, Z), on the host
static int ibm_masks(fl_ibm *m, const RouteP &R, int64_t L, const double *X, const double *Y, const double *Z, std::vector<int> &host)
{
  fl_poisson *h = m->gp;
  host.assign((size_t)L, 0);
  if (L == 0) return 0;
  FL_CHK(ibm_reserve(h, &m->mask, &m->maskcap, L));
  IbmP P = m->P;
  P.L    = L;
  hipLaunchKernelGGL(k_ibm_route, dim3((unsigned)((L + 255) / 256)), dim3(256), 0, h->stream, P, R, X, Y, Z, m->mask);
  FL_HIP(hipGetLastError());
  FL_HIP(hipMemcpyAsync(host.data(), m->mask, sizeof(int) * (size_t)L, hipMemcpyDeviceToHost, h->stream));
  FL_HIP(hipStreamSynchronize(h->stream));
  return 0;
}

// The messages of one exchange between owners and ghost holders.  to_ghosts: the owners send (spread, positions), else the ghost holders
// do (interp).  per = doubles per copy.  Sends in ascending offset code; receives in the order the peer sends, which is DESCENDING code
// here (the peer numbers the same pair of blocks 26 - code): RCCL matches the messages between two ranks by order, and two offsets may
// lead to the same rank (two ranks on a periodic axis) -- fl_halo_plan's rule.  Empty messages are left out: both sides know every count.
static void ibm_msgs(const fl_ibm *m, bool to_ghosts, int per, double *sbuf, double *rbuf, std::vector<Msg> &msgs)
{
  const int *sc = to_ghosts ? m->scnt : m->gcnt, *so = to_ghosts ? m->soff : m->goff;
  const int *rc = to_ghosts ? m->gcnt : m->scnt, *ro = to_ghosts ? m->goff : m->soff;
  msgs.clear();
  for (int code = 0; code < 27; ++code)
    if (m->peer[code] >= 0 && sc[code] > 0) msgs.push_back({m->peer[code], sbuf + (int64_t)per * so[code], nullptr, (int64_t)per * sc[code], code, 26 - code});
  for (int code = 26; code >= 0; --code)
    if (m->peer[code] >= 0 && rc[code] > 0) msgs.push_back({m->peer[code], nullptr, rbuf + (int64_t)per * ro[code], (int64_t)per * rc[code], code, 26 - code});
}

// own markers (Lo of them, the caller's device arrays) -> ghost copies on the neighbours, marker arrays of own + ghost, bins.  Collective.
static int ibm_route(fl_ibm *m, int64_t Lo, const double *X, const double *Y, const double *Z, const int64_t *gid_new, bool first)
{
  fl_poisson *h = m->gp;
  hipStream_t s = h->stream;
  const IbmP &P = m->P;
  const bool  split = ibm_split(h);
  // which offsets have a rank behind them
  RouteP R;
  int    periodic[3];
  for (int d = 0; d < 3; ++d) {
    periodic[d]  = P.periodic[d];
    const bool sp = h->dec.ranks[d] > 1;
    R.peer_lo[d] = sp && (h->dec.coord[d] > 0 || P.periodic[d]);
    R.peer_hi[d] = sp && (h->dec.coord[d] < h->dec.ranks[d] - 1 || P.periodic[d]);
  }
  int peer[27];
  for (int code = 0; code < 27; ++code) {
    const int o[3] = {code % 3 - 1, (code / 3) % 3 - 1, code / 9 - 1};
    bool      ok   = code != 13;
    for (int d = 0; d < 3; ++d) ok = ok && (o[d] == 0 || (o[d] < 0 ? R.peer_lo[d] : R.peer_hi[d]));
    peer[code] = ok ? fl_decomp_neighbor_offset(&h->dec, periodic, o) : -1;
  }
  // every marker in its owner's block, every split axis >= 4 cells long: or every rank leaves here with the same error
  std::vector<int> mask;
  FL_CHK(ibm_masks(m, R, Lo, X, Y, Z, mask));
  double vote[3] = {0., gid_new ? 1. : 0., (!gid_new && Lo > 0) ? 1. : 0.};
  for (int64_t l = 0; l < Lo; ++l)
    if (mask[(size_t)l] < 0) vote[0] = 1.;
  for (int d = 0; d < 3; ++d)
    if (h->dec.ranks[d] > 1 && P.n[d] < 4) vote[0] = 1.;
  if (!first) vote[1] = vote[2] = 0.;  // update keeps the numbers given at create
  FL_CHK(ibm_vote(h, vote, 3));
  if (vote[0] > 0.) return FL_ERR_ARG_OUTOFRANGE;
  if (first) {
    if (vote[1] > 0. && vote[2] > 0.) return FL_ERR_ARG_WRONG;  // marker numbers on some ranks only
    m->has_gid = vote[1] > 0.;
  }
  // send list: the own markers of every offset in ascending local order, offsets in ascending code; per marker the copies it has
  std::vector<int> sendlist, cstart((size_t)Lo + 1, 0), clist;
  for (int code = 0; code < 27; ++code) {
    m->peer[code] = peer[code];
    m->soff[code] = (int)sendlist.size();
    if (peer[code] >= 0)
      for (int64_t l = 0; l < Lo; ++l)
        if (mask[(size_t)l] >> code & 1) {
          sendlist.push_back((int)l);
          cstart[(size_t)l + 1]++;
        }
    m->scnt[code] = (int)sendlist.size() - m->soff[code];
    m->gcnt[code] = m->goff[code] = 0;
  }
  const int ncopy = (int)sendlist.size();
  for (int64_t l = 0; l < Lo; ++l) cstart[(size_t)l + 1] += cstart[(size_t)l];
  clist.resize((size_t)ncopy);
  {
    std::vector<int> cur(cstart.begin(), cstart.end() - 1);
    for (int j = 0; j < ncopy; ++j) clist[(size_t)cur[(size_t)sendlist[(size_t)j]]++] = j;  // ascending j per marker
  }
  m->Lo    = Lo;
  m->ncopy = ncopy;
  m->R     = R;
  ibm_free(h, &m->sendlist);
  ibm_free(h, &m->cstart);
  ibm_free(h, &m->clist);
  if (fl_dev_alloc(h, (void **)&m->sendlist, sizeof(int) * (size_t)ncopy, false) || fl_dev_alloc(h, (void **)&m->cstart, sizeof(int) * ((size_t)Lo + 1), false) || fl_dev_alloc(h, (void **)&m->clist, sizeof(int) * (size_t)ncopy, false))
    return FL_ERR_MEM;
  if (ncopy) FL_HIP(hipMemcpyAsync(m->sendlist, sendlist.data(), sizeof(int) * (size_t)ncopy, hipMemcpyHostToDevice, s));
  if (ncopy) FL_HIP(hipMemcpyAsync(m->clist, clist.data(), sizeof(int) * (size_t)ncopy, hipMemcpyHostToDevice, s));
  FL_HIP(hipMemcpyAsync(m->cstart, cstart.data(), sizeof(int) * ((size_t)Lo + 1), hipMemcpyHostToDevice, s));
  if (first && m->has_gid && Lo > 0) {
    if (fl_dev_alloc(h, (void **)&m->gid_own, sizeof(int64_t) * (size_t)Lo, false)) return FL_ERR_MEM;
    m->gidowncap = Lo;
    FL_HIP(hipMemcpyAsync(m->gid_own, gid_new, sizeof(int64_t) * (size_t)Lo, hipMemcpyDeviceToDevice, s));
  }
  // the counts of the copies, one double per offset that has a rank behind it
  int64_t Lg = 0;
  if (split) {
    if (!m->cbuf && fl_dev_alloc(h, (void **)&m->cbuf, sizeof(double) * 54, true)) return FL_ERR_MEM;
    double hc[54];
    for (int code = 0; code < 27; ++code) hc[code] = (double)m->scnt[code], hc[27 + code] = 0.;
    FL_HIP(hipMemcpyAsync(m->cbuf, hc, sizeof(hc), hipMemcpyHostToDevice, s));
    std::vector<Msg> msgs;
    for (int code = 0; code < 27; ++code)
      if (peer[code] >= 0) msgs.push_back({peer[code], m->cbuf + code, nullptr, 1, code, 26 - code});
    for (int code = 26; code >= 0; --code)
      if (peer[code] >= 0) msgs.push_back({peer[code], nullptr, m->cbuf + 27 + code, 1, code, 26 - code});
    FL_CHK(h->comm.exchange(s, msgs));
    FL_HIP(hipMemcpyAsync(hc, m->cbuf, sizeof(hc), hipMemcpyDeviceToHost, s));
    FL_HIP(hipStreamSynchronize(s));  // the sendlist vectors above are still alive here
    for (int code = 0; code < 27; ++code) {
      m->goff[code] = (int)Lg;
      m->gcnt[code] = peer[code] >= 0 ? (int)hc[27 + code] : 0;
      Lg += m->gcnt[code];
    }
  } else FL_HIP(hipStreamSynchronize(s));
  m->Lg             = Lg;
  const int64_t Lt = Lo + Lg;
  if (Lt > (int64_t)1 << 27) return FL_ERR_ARG_OUTOFRANGE;
  m->P.L = Lt;
  FL_CHK(ibm_alloc_markers(m, Lt));
  if (Lo > 0) {
    FL_HIP(hipMemcpyAsync(m->X, X, sizeof(double) * (size_t)Lo, hipMemcpyDeviceToDevice, s));
    FL_HIP(hipMemcpyAsync(m->Y, Y, sizeof(double) * (size_t)Lo, hipMemcpyDeviceToDevice, s));
    FL_HIP(hipMemcpyAsync(m->Z, Z, sizeof(double) * (size_t)Lo, hipMemcpyDeviceToDevice, s));
    if (m->has_gid) FL_HIP(hipMemcpyAsync(m->gid, m->gid_own, sizeof(int64_t) * (size_t)Lo, hipMemcpyDeviceToDevice, s));
  }
  // positions (and numbers) of the copies
  if (ncopy > 0 || Lg > 0) {
    FL_CHK(ibm_reserve(h, &m->sbuf, &m->sbufcap, 4 * (int64_t)ncopy));
    FL_CHK(ibm_reserve(h, &m->rbuf, &m->rbufcap, 4 * Lg));
    if (ncopy > 0) hipLaunchKernelGGL(k_ibm_pack_pos, dim3((ncopy + 255) / 256), dim3(256), 0, s, ncopy, m->sendlist, m->X, m->Y, m->Z, (const int64_t *)(m->has_gid ? m->gid : nullptr), m->sbuf);
    std::vector<Msg> msgs;
    ibm_msgs(m, true, 4, m->sbuf, m->rbuf, msgs);
    FL_CHK(h->comm.exchange(s, msgs));
    if (Lg > 0) hipLaunchKernelGGL(k_ibm_unpack_pos, dim3((unsigned)((Lg + 255) / 256)), dim3(256), 0, s, (int)Lg, Lo, m->rbuf, m->X, m->Y, m->Z, m->has_gid ? m->gid : nullptr);
    FL_HIP(hipGetLastError());
  }
  return ibm_rebin(m);
}

extern "C" int fl_ibm_owned_select(fl_poisson *h, int kind, int64_t L, const double *X, const double *Y, const double *Z, int64_t *idx_out_dev, int64_t *count_out)
{
  if (!h || !X || !Y || !Z || !idx_out_dev || !count_out) return FL_ERR_ARG_NULL;
  if (kind != FL_DELTA_PESKIN4 && kind != FL_DELTA_ROMA3) return FL_ERR_ARG_OUTOFRANGE;
  if (L < 1 || L > (int64_t)1 << 27) return FL_ERR_ARG_OUTOFRANGE;
  FL_HIP(hipSetDevice(h->device));
  fl_ibm m;  // geometry and the mask buffer only
  m.gp   = h;
  int rc = ibm_geometry(h, kind, m.P, m.xcg);
  std::vector<int>     mask;
  std::vector<int64_t> idx;
  const RouteP         none = {{0, 0, 0}, {0, 0, 0}};
  if (!rc) rc = ibm_masks(&m, none, L, X, Y, Z, mask);
  if (!rc) {
    for (int64_t l = 0; l < L; ++l)
      if (mask[(size_t)l] >= 0) idx.push_back(l);
    if (!idx.empty() && hipMemcpyAsync(idx_out_dev, idx.data(), sizeof(int64_t) * idx.size(), hipMemcpyHostToDevice, h->stream) != hipSuccess) rc = FL_ERR_GPU;
    if (hipStreamSynchronize(h->stream) != hipSuccess) rc = FL_ERR_GPU;
    *count_out = (int64_t)idx.size();
  }
  for (void *p : {(void *)m.mask, (void *)m.xcg[0], (void *)m.xcg[1], (void *)m.xcg[2]})
    if (p) (void)hipFree(p);
  return rc;
}

extern "C" int fl_ibm_create_owned(fl_poisson *h, int kind, int64_t L_local, const double *X, const double *Y, const double *Z, const int64_t *gid_dev, fl_ibm **out)
{
  if (!h || !out) return FL_ERR_ARG_NULL;
  *out = nullptr;
  // argument errors of one rank are voted like a misplaced marker: the others must not wait in an exchange this rank never enters
  int bad = 0;
  if (L_local > 0 && (!X || !Y || !Z)) bad = FL_ERR_ARG_NULL;
  if (kind != FL_DELTA_PESKIN4 && kind != FL_DELTA_ROMA3) bad = FL_ERR_ARG_OUTOFRANGE;
  if (L_local < 0 || L_local > (int64_t)1 << 27) bad = FL_ERR_ARG_OUTOFRANGE;
  FL_HIP(hipSetDevice(h->device));
  fl_ibm *m = nullptr;
  if (!bad) bad = ibm_new(h, kind, true, &m);
  double v = bad ? 1. : 0.;
  const int vrc = ibm_vote(h, &v, 1);
  if (vrc || v > 0.) {
    if (m) fl_ibm_destroy(m);
    return vrc ? vrc : (bad ? bad : FL_ERR_ARG_OUTOFRANGE);
  }
  const int rc = ibm_route(m, L_local, X, Y, Z, L_local > 0 ? gid_dev : nullptr, true);
  if (rc) {
    fl_ibm_destroy(m);
    return rc;
  }
  *out = m;
  return FL_SUCCESS;
}

extern "C" int fl_ibm_owned_counts(fl_ibm *m, int64_t out[5])
{
  if (!m || !out) return FL_ERR_ARG_NULL;
  if (!m->owned) return FL_ERR_ARG_WRONGSTATE;
  out[0] = m->Lo;
  out[1] = m->Lg;
  out[2] = m->ncopy;
  out[3] = 8 * m->Lg;                   // interp: one double per ghost and component back to its owner
  out[4] = 32 * (int64_t)m->ncopy;      // spread of three components: (F_0, F_1, F_2, dV) per copy
  return FL_SUCCESS;
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
  FL_HIP(hipMemcpyAsync(m->X, X, sizeof(double) * m->P.L, hipMemcpyDeviceToDevice, h->stream));
  FL_HIP(hipMemcpyAsync(m->Y, Y, sizeof(double) * m->P.L, hipMemcpyDeviceToDevice, h->stream));
  FL_HIP(hipMemcpyAsync(m->Z, Z, sizeof(double) * m->P.L, hipMemcpyDeviceToDevice, h->stream));
  return ibm_rebin(m);
}

// ---- owner-rank markers: migration ----------------------------------------------------------------------------------------------------

// the cell ranges of the blocks behind the six faces: every rank tells its face neighbours (lo, n) of its block, once per set
static int ibm_neighbour_ranges(fl_ibm *m)
{
  fl_poisson *h = m->gp;
  hipStream_t s = h->stream;
  const IbmP &P = m->P;
  DestP      &D = m->D;
  for (int d = 0; d < 3; ++d) {
    D.peer_lo[d] = m->R.peer_lo[d];
    D.peer_hi[d] = m->R.peer_hi[d];
    D.lo_beg[d] = D.lo_end[d] = D.hi_beg[d] = D.hi_end[d] = 0;
  }
  m->nbr_known = true;
  if (!ibm_split(h)) return 0;
  if (!m->nbuf && fl_dev_alloc(h, (void **)&m->nbuf, sizeof(double) * 6 * 28, true)) return FL_ERR_MEM;
  double hb[6 * 28] = {0.};
  for (int d = 0; d < 3; ++d) hb[d] = (double)P.lo[d], hb[3 + d] = (double)P.n[d];
  FL_HIP(hipMemcpyAsync(m->nbuf, hb, sizeof(double) * 6, hipMemcpyHostToDevice, s));
  const int        face[6] = {12, 14, 10, 16, 4, 22};  // ascending below: 4, 10, 12, 14, 16, 22
  std::vector<Msg> msgs;
  for (int code = 0; code < 27; ++code)
    for (int f = 0; f < 6; ++f)
      if (face[f] == code && m->peer[code] >= 0) msgs.push_back({m->peer[code], m->nbuf, nullptr, 6, code, 26 - code});
  for (int code = 26; code >= 0; --code)
    for (int f = 0; f < 6; ++f)
      if (face[f] == code && m->peer[code] >= 0) msgs.push_back({m->peer[code], nullptr, m->nbuf + 6 * (1 + code), 6, code, 26 - code});
  FL_CHK(h->comm.exchange(s, msgs));
  FL_HIP(hipMemcpyAsync(hb, m->nbuf, sizeof(hb), hipMemcpyDeviceToHost, s));
  FL_HIP(hipStreamSynchronize(s));
  for (int d = 0; d < 3; ++d) {
    const int step = d == 0 ? 1 : (d == 1 ? 3 : 9), lo = 13 - step, hi = 13 + step;
    if (m->peer[lo] >= 0) D.lo_beg[d] = (int)hb[6 * (1 + lo) + d], D.lo_end[d] = D.lo_beg[d] + (int)hb[6 * (1 + lo) + 3 + d];
    if (m->peer[hi] >= 0) D.hi_beg[d] = (int)hb[6 * (1 + hi) + d], D.hi_end[d] = D.hi_beg[d] + (int)hb[6 * (1 + hi) + 3 + d];
  }
  return 0;
}

extern "C" int fl_ibm_migrate(fl_ibm *m, const double *X, const double *Y, const double *Z, int nattr, const double *attr_dev, int64_t *L_local_new, int64_t moved[2])
{
  if (!m) return FL_ERR_ARG_NULL;
  if (!m->owned || !m->has_gid) return FL_ERR_ARG_WRONGSTATE;  // has_gid was voted at create: the same on every rank
  fl_poisson   *h  = m->gp;
  hipStream_t   s  = h->stream;
  const int64_t Lo = m->Lo;
  FL_HIP(hipSetDevice(h->device));
  const bool nattr_ok = nattr >= 0 && nattr <= 8;
  const bool null_arg = !L_local_new || !moved || (Lo > 0 && (!X || !Y || !Z || (nattr_ok && nattr > 0 && !attr_dev)));
  double     v[2]     = {nattr_ok ? 0. : 1., null_arg ? 1. : 0.};
  FL_CHK(ibm_vote(h, v, 2));
  if (v[0] > 0.) return FL_ERR_ARG_OUTOFRANGE;
  if (v[1] > 0.) return FL_ERR_ARG_NULL;
  if (!m->nbr_known) FL_CHK(ibm_neighbour_ranges(m));
  // 1. where every own marker goes; the 27 counts, the two flags
  const int nb = (int)((Lo + 255) / 256);
  if (!m->mcnt && fl_dev_alloc(h, (void **)&m->mcnt, sizeof(int) * (MIG_NCNT + 28 + 27), true)) return FL_ERR_MEM;
  int hc[MIG_NCNT] = {0};
  if (Lo > 0) {
    FL_CHK(ibm_reserve(h, &m->dest, &m->destcap, Lo));
    FL_CHK(ibm_reserve(h, &m->bstay, &m->bstaycap, nb + 1));
    FL_CHK(ibm_reserve(h, &m->boff, &m->boffcap, nb + 1));
    FL_HIP(hipMemsetAsync(m->mcnt, 0, sizeof(int) * (MIG_NCNT + 28 + 27), s));
    IbmP P = m->P;
    P.L    = Lo;
    hipLaunchKernelGGL(k_ibm_dest, dim3(nb), dim3(256), 0, s, P, m->D, X, Y, Z, (const int64_t *)m->gid_own, m->dest, m->mcnt, m->bstay);
    FL_HIP(hipGetLastError());
    FL_HIP(hipMemcpyAsync(hc, m->mcnt, sizeof(hc), hipMemcpyDeviceToHost, s));
    FL_HIP(hipStreamSynchronize(s));
  }
  // 2. the votes, then the counts to and from the neighbours (ibm_route's count messages)
  double bad[2] = {hc[28] ? 1. : 0., hc[27] > 0 ? 1. : 0.};
  FL_CHK(ibm_vote(h, bad, 2));
  if (bad[0] > 0.) return FL_ERR_ARG_WRONGSTATE;
  if (bad[1] > 0.) return FL_ERR_ARG_OUTOFRANGE;
  int     lcnt[27], loff[28], acnt[27], aoff[28];
  int64_t nleave = 0, A = 0;
  for (int code = 0; code < 27; ++code) {
    lcnt[code] = (code != 13 && m->peer[code] >= 0) ? hc[code] : 0;  // a code without a peer holds nothing: k_ibm_dest never forms it
    loff[code] = (int)nleave;
    nleave += lcnt[code];
    acnt[code] = 0;
  }
  loff[27] = (int)nleave;
  if (ibm_split(h)) {
    double hd[54];
    for (int code = 0; code < 27; ++code) hd[code] = (double)lcnt[code], hd[27 + code] = 0.;
    FL_HIP(hipMemcpyAsync(m->cbuf, hd, sizeof(hd), hipMemcpyHostToDevice, s));
    std::vector<Msg> msgs;
    for (int code = 0; code < 27; ++code)
      if (m->peer[code] >= 0) msgs.push_back({m->peer[code], m->cbuf + code, nullptr, 1, code, 26 - code});
    for (int code = 26; code >= 0; --code)
      if (m->peer[code] >= 0) msgs.push_back({m->peer[code], nullptr, m->cbuf + 27 + code, 1, code, 26 - code});
    FL_CHK(h->comm.exchange(s, msgs));
    FL_HIP(hipMemcpyAsync(hd, m->cbuf, sizeof(hd), hipMemcpyDeviceToHost, s));
    FL_HIP(hipStreamSynchronize(s));
    for (int code = 0; code < 27; ++code) acnt[code] = m->peer[code] >= 0 ? (int)hd[27 + code] : 0;
  }
  for (int code = 0; code < 27; ++code) aoff[code] = (int)A, A += acnt[code];
  aoff[27]          = (int)A;
  const int64_t Ls = Lo - nleave, Ln = Ls + A;
  if (Ln > (int64_t)1 << 27) return FL_ERR_ARG_OUTOFRANGE;
  m->nattr = nattr;
  if (nleave == 0 && A == 0) {
    // nothing crosses a face of this block: the list stays as it is, only the attributes are kept for fl_ibm_owned_fetch
    if (nattr > 0 && Lo > 0) {
      FL_CHK(ibm_reserve(h, &m->attr, &m->attrcap, (int64_t)nattr * Lo));
      FL_HIP(hipMemcpyAsync(m->attr, attr_dev, sizeof(double) * (size_t)nattr * (size_t)Lo, hipMemcpyDeviceToDevice, s));
    }
    *L_local_new = Lo;
    moved[0] = moved[1] = 0;
    return ibm_route(m, Lo, X, Y, Z, nullptr, false);
  }
  const int per = 4 + nattr;
  FL_CHK(ibm_reserve(h, &m->sbuf, &m->sbufcap, per * nleave));
  FL_CHK(ibm_reserve(h, &m->rbuf, &m->rbufcap, per * A));
  FL_CHK(ibm_reserve(h, &m->stay, &m->staycap, per * Ls));
  FL_CHK(ibm_reserve(h, &m->arr, &m->arrcap, per * A));
  FL_CHK(ibm_reserve(h, &m->mpos, &m->mposcap, 3 * Ln));
  FL_CHK(ibm_reserve(h, &m->gidtmp, &m->gidtmpcap, Ln));
  FL_CHK(ibm_reserve(h, &m->attrtmp, &m->attrtmpcap, (int64_t)nattr * Ln));
  // 3. + 4. stayers compacted in order, leavers packed by offset
  if (Lo > 0) {
    int *leaveoff = m->mcnt + MIG_NCNT, *cursor = m->mcnt + MIG_NCNT + 28;
    FL_HIP(hipMemcpyAsync(leaveoff, loff, sizeof(loff), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_ibm_scan, dim3(1), dim3(256), 0, s, m->bstay, m->boff, nb);
    hipLaunchKernelGGL(k_ibm_split, dim3(nb), dim3(256), 0, s, Lo, Ls, nattr, m->dest, m->boff, leaveoff, cursor, X, Y, Z, (const int64_t *)m->gid_own, attr_dev, m->stay, m->sbuf);
    FL_HIP(hipGetLastError());
  }
  // 5. one exchange: a message per offset, ibm_msgs' ordering rule
  {
    std::vector<Msg> msgs;
    for (int code = 0; code < 27; ++code)
      if (m->peer[code] >= 0 && lcnt[code] > 0) msgs.push_back({m->peer[code], m->sbuf + (int64_t)per * loff[code], nullptr, (int64_t)per * lcnt[code], code, 26 - code});
    for (int code = 26; code >= 0; --code)
      if (m->peer[code] >= 0 && acnt[code] > 0) msgs.push_back({m->peer[code], nullptr, m->rbuf + (int64_t)per * aoff[code], (int64_t)per * acnt[code], code, 26 - code});
    FL_CHK(h->comm.exchange(s, msgs));
  }
  // 6. + 7. arrivals by number, then both ascending lists into one
  if (A > 0) hipLaunchKernelGGL(k_ibm_rank_arrivals, dim3((unsigned)((A + 255) / 256)), dim3(256), 0, s, (int)A, per, m->rbuf, m->arr);
  if (Ln > 0) hipLaunchKernelGGL(k_ibm_merge, dim3((unsigned)((Ln + 255) / 256)), dim3(256), 0, s, Ls, A, nattr, m->stay, m->arr, m->mpos, m->gidtmp, m->attrtmp);
  FL_HIP(hipGetLastError());
  std::swap(m->gid_own, m->gidtmp);
  std::swap(m->gidowncap, m->gidtmpcap);
  std::swap(m->attr, m->attrtmp);
  std::swap(m->attrcap, m->attrtmpcap);
  *L_local_new = Ln;
  moved[0]     = nleave;
  moved[1]     = A;
  // 8. ghost copies and bins of the new own list
  return ibm_route(m, Ln, m->mpos, m->mpos + Ln, m->mpos + 2 * Ln, nullptr, false);
}

extern "C" int fl_ibm_owned_fetch(fl_ibm *m, int64_t cap, double *X, double *Y, double *Z, int64_t *gid, int nattr, double *attr_out)
{
  if (!m) return FL_ERR_ARG_NULL;
  if (!m->owned) return FL_ERR_ARG_WRONGSTATE;
  if (cap < m->Lo) return FL_ERR_ARG_SIZ;
  if (nattr < 0 || nattr > m->nattr) return FL_ERR_ARG_OUTOFRANGE;
  if (gid && !m->has_gid) return FL_ERR_ARG_WRONGSTATE;
  if (nattr > 0 && !attr_out && m->Lo > 0) return FL_ERR_ARG_NULL;
  fl_poisson  *h = m->gp;
  hipStream_t  s = h->stream;
  const size_t n = (size_t)m->Lo;
  FL_HIP(hipSetDevice(h->device));
  if (n == 0) return FL_SUCCESS;
  if (X) FL_HIP(hipMemcpyAsync(X, m->X, sizeof(double) * n, hipMemcpyDeviceToDevice, s));
  if (Y) FL_HIP(hipMemcpyAsync(Y, m->Y, sizeof(double) * n, hipMemcpyDeviceToDevice, s));
  if (Z) FL_HIP(hipMemcpyAsync(Z, m->Z, sizeof(double) * n, hipMemcpyDeviceToDevice, s));
  if (gid) FL_HIP(hipMemcpyAsync(gid, m->gid_own, sizeof(int64_t) * n, hipMemcpyDeviceToDevice, s));
  if (nattr > 0) FL_HIP(hipMemcpyAsync(attr_out, m->attr, sizeof(double) * n * (size_t)nattr, hipMemcpyDeviceToDevice, s));
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

// ---- owner-rank markers: per call (stream-ordered; the host waits only where the host transport itself does) ---------------------------

static int ibm_interp_owned(fl_ibm *m, int ncomp, const double *u, double *U)
{
  fl_poisson   *h  = m->gp;
  hipStream_t   s  = h->stream;
  const int64_t Lo = m->Lo, Lg = m->Lg, Lt = Lo + Lg;
  if (Lo > 0 && !U) return FL_ERR_ARG_NULL;
  if (Lt == 0) return FL_SUCCESS;
  FL_CHK(ibm_reserve(h, &m->Ui, &m->Uicap, (int64_t)ncomp * Lt));
  FL_CHK(ibm_reserve(h, &m->sbuf, &m->sbufcap, (int64_t)ncomp * Lg));
  FL_CHK(ibm_reserve(h, &m->rbuf, &m->rbufcap, (int64_t)ncomp * m->ncopy));
  hipLaunchKernelGGL(k_ibm_interp, dim3((unsigned)((Lt + 3) / 4)), dim3(256), 0, s, m->P, m->i0, m->w, ncomp, h->ncell, u, m->Ui);
  if (Lg > 0) hipLaunchKernelGGL(k_ibm_pack_U, dim3((unsigned)((Lg + 255) / 256)), dim3(256), 0, s, (int)Lg, Lo, Lt, ncomp, m->Ui, m->sbuf);
  FL_HIP(hipGetLastError());
  if (Lg > 0 || m->ncopy > 0) {
    std::vector<Msg> msgs;
    ibm_msgs(m, false, ncomp, m->sbuf, m->rbuf, msgs);
    FL_CHK(h->comm.exchange(s, msgs));
  }
  if (Lo > 0) hipLaunchKernelGGL(k_ibm_collect_U, dim3((unsigned)((Lo + 255) / 256)), dim3(256), 0, s, Lo, Lt, ncomp, m->Ui, m->cstart, m->clist, m->rbuf, U);
  FL_HIP(hipGetLastError());
  return FL_SUCCESS;
}

// one: the one-component kernel of the scalar forcing (ncomp = 1), else fl_ibm_spread's
static int ibm_spread_owned(fl_ibm *m, int ncomp, const double *F, const double *dV, double *f, bool one = false)
{
  fl_poisson   *h  = m->gp;
  hipStream_t   s  = h->stream;
  const int64_t Lo = m->Lo, Lg = m->Lg, Lt = Lo + Lg;
  if (Lo > 0 && (!F || !dV)) return FL_ERR_ARG_NULL;
  if (Lt == 0) return FL_SUCCESS;
  const int per = ncomp + 1;
  FL_CHK(ibm_reserve(h, &m->Fi, &m->Ficap, (int64_t)per * Lt));
  FL_CHK(ibm_reserve(h, &m->sbuf, &m->sbufcap, (int64_t)per * m->ncopy));
  FL_CHK(ibm_reserve(h, &m->rbuf, &m->rbufcap, (int64_t)per * Lg));
  if (m->ncopy > 0) hipLaunchKernelGGL(k_ibm_pack_F, dim3((m->ncopy + 255) / 256), dim3(256), 0, s, m->ncopy, Lo, ncomp, m->sendlist, F, dV, m->sbuf);
  FL_HIP(hipGetLastError());
  if (Lg > 0 || m->ncopy > 0) {
    std::vector<Msg> msgs;
    ibm_msgs(m, true, per, m->sbuf, m->rbuf, msgs);
    FL_CHK(h->comm.exchange(s, msgs));
  }
  double *Fi = m->Fi, *dVi = m->Fi + (int64_t)ncomp * Lt;
  hipLaunchKernelGGL(k_ibm_stage_F, dim3((unsigned)((Lt + 255) / 256)), dim3(256), 0, s, Lo, Lt, ncomp, F, dV, m->rbuf, Fi, dVi);
  if (m->nactive > 0 && one) hipLaunchKernelGGL(k_ibm_spread<1>, dim3(m->nactive), dim3(256), 0, s, m->P, m->i0, m->w, m->off, m->list, m->active, 1, h->ncell, Fi, dVi, f);
  else if (m->nactive > 0) hipLaunchKernelGGL(k_ibm_spread<3>, dim3(m->nactive), dim3(256), 0, s, m->P, m->i0, m->w, m->off, m->list, m->active, ncomp, h->ncell, Fi, dVi, f);
  FL_HIP(hipGetLastError());
  return FL_SUCCESS;
}

extern "C" int fl_ibm_interp(fl_ibm *m, int ncomp, const double *u, double *U)
{
  if (!m || !u) return FL_ERR_ARG_NULL;
  if (ncomp < 1) return FL_ERR_ARG_OUTOFRANGE;
  fl_poisson *h = m->gp;
  FL_HIP(hipSetDevice(h->device));
  if (m->owned) return ibm_interp_owned(m, ncomp, u, U);
  if (!U) return FL_ERR_ARG_NULL;
  hipLaunchKernelGGL(k_ibm_interp, dim3((unsigned)((m->P.L + 3) / 4)), dim3(256), 0, h->stream, m->P, m->i0, m->w, ncomp, h->ncell, u, U);
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
  if (m->nactive > 0) hipLaunchKernelGGL(k_ibm_spread<3>, dim3(m->nactive), dim3(256), 0, h->stream, m->P, m->i0, m->w, m->off, m->list, m->active, ncomp, h->ncell, F, dV, f);
  FL_HIP(hipGetLastError());
  return FL_SUCCESS;
}

// ---- force and torque on each body --------------------------------------------------------------------------------------------------------

extern "C" int fl_ibm_force(fl_ibm *m, const double *F, const double *dV, const int32_t *body, int nbody, const double *about, double *force, double *torque)
{
  if (!m) return FL_ERR_ARG_NULL;
  fl_poisson   *h     = m->gp;
  hipStream_t   s     = h->stream;
  const bool    coll  = m->owned && ibm_split(h);  // an owned set on several ranks: collective, every error is voted
  const int64_t L     = m->owned ? m->Lo : m->P.L;
  const bool    null_arg = !force || !about || (L > 0 && (!F || !dV));
  const bool    nbody_ok = nbody >= 1 && nbody <= FORCE_MAXBODY;
  FL_HIP(hipSetDevice(h->device));
  double Lglob = (double)L;
  bool   anybody = body != nullptr;
  if (coll) {
    double v[4] = {null_arg ? 1. : 0., nbody_ok ? 0. : 1., (double)L, body ? 1. : 0.};
    FL_CHK(ibm_vote(h, v, 4));
    if (v[0] > 0.) return FL_ERR_ARG_NULL;
    if (v[1] > 0.) return FL_ERR_ARG_OUTOFRANGE;
    Lglob   = v[2];
    anybody = v[3] > 0.;  // a rank without markers may leave the body array out: every rank still reduces the same number of sums
  } else {
    if (null_arg) return FL_ERR_ARG_NULL;
    if (!nbody_ok) return FL_ERR_ARG_OUTOFRANGE;
  }
  if (Lglob >= (double)((int64_t)1 << 22)) return FL_ERR_SUP;  // beyond it the integer sums could leave the 53 bits of a double
  const int nbk = body ? nbody : 1;     // bodies the kernels index on this rank
  const int nb  = anybody ? nbody : 1;  // bodies the sums are kept for
  const int n   = 12 * nb;
  std::vector<double> host((size_t)(FW_SUMS + n), 0.);
  if (L > 0) {
    if (!m->fws && fl_dev_alloc(h, (void **)&m->fws, sizeof(double) * FW_END, true)) return FL_ERR_MEM;
    if (!m->ftick && fl_dev_alloc(h, (void **)&m->ftick, 16, true)) return FL_ERR_MEM;
  }
  ForceP Q;
  Q.L     = L;
  Q.nbody = nbk;
  for (int d = 0; d < 3; ++d) {
    const Axis &A  = h->ax[d];
    Q.periodic[d] = A.periodic ? 1 : 0;
    Q.per[d]      = A.xf[A.n] - A.xf[0];
    Q.about[d]    = about[d];
  }
  const int nblk = (int)std::min<int64_t>((L + 255) / 256, FORCE_MAXBLK);
  if (L > 0) {
    FL_HIP(hipMemsetAsync(m->ftick, 0, 16, s));
    if (body) FL_HIP(hipMemcpyAsync(m->fws + FW_ABOUT, about, sizeof(double) * 3 * (size_t)nbk, hipMemcpyHostToDevice, s));
    if (body) hipLaunchKernelGGL(k_ibm_force_max<true>, dim3(nblk), dim3(256), 0, s, Q, m->X, m->Y, m->Z, F, dV, body, m->fws, m->ftick);
    else hipLaunchKernelGGL(k_ibm_force_max<false>, dim3(nblk), dim3(256), 0, s, Q, m->X, m->Y, m->Z, F, dV, body, m->fws, m->ftick);
    FL_HIP(hipGetLastError());
  }
  if (coll) {
    // the two maxima and the flag over the ranks, then back to the device: every rank splits by the same E
    if (L > 0) {
      FL_HIP(hipMemcpyAsync(host.data(), m->fws, sizeof(double) * 4, hipMemcpyDeviceToHost, s));
      FL_HIP(hipStreamSynchronize(s));
    }
    FL_CHK(fl_allreduce_max(h, &host[0]));
    FL_CHK(fl_allreduce_max(h, &host[1]));
    FL_CHK(ibm_vote(h, &host[2], 1));
    if (host[2] > 0.) return FL_ERR_ARG_OUTOFRANGE;
    if (L > 0) FL_HIP(hipMemcpyAsync(m->fws, host.data(), sizeof(double) * 2, hipMemcpyHostToDevice, s));
  }
  if (L > 0) {
    if (body) hipLaunchKernelGGL(k_ibm_force_sum<true>, dim3(nblk), dim3(256), 0, s, Q, m->X, m->Y, m->Z, F, dV, body, m->fws, m->ftick + 1);
    else hipLaunchKernelGGL(k_ibm_force_sum<false>, dim3(nblk), dim3(256), 0, s, Q, m->X, m->Y, m->Z, F, dV, body, m->fws, m->ftick + 1);
    FL_HIP(hipGetLastError());
    const double amax[2] = {host[0], host[1]};
    FL_HIP(hipMemcpyAsync(host.data(), m->fws, sizeof(double) * (size_t)(FW_SUMS + 12 * nbk), hipMemcpyDeviceToHost, s));
    FL_HIP(hipStreamSynchronize(s));  // the one host wait of a call on one rank
    if (coll) host[0] = amax[0], host[1] = amax[1];
    else if (host[2] > 0.) return FL_ERR_ARG_OUTOFRANGE;
  }
  if (coll)  // sums of exact integers stay exact: eight at a time through the handle's sum all-reduce
    for (int j = 0; j < n; j += 8) FL_CHK(fl_poisson_allreduce_sum(h, &host[(size_t)(FW_SUMS + j)], std::min(8, n - j)));
  for (int b = 0; b < nbody; ++b)
    for (int c = 0; c < 3; ++c) {
      const double *q = &host[(size_t)(FW_SUMS + 12 * (b < nb ? b : 0))];
      force[3 * b + c] = b < nb ? force_combine(host[0], q[2 * c], q[2 * c + 1]) : (host[0] <= 1.7976931348623157e308 ? 0. : std::nan(""));
      if (torque) torque[3 * b + c] = b < nb ? force_combine(host[1], q[2 * (3 + c)], q[2 * (3 + c) + 1]) : (host[1] <= 1.7976931348623157e308 ? 0. : std::nan(""));
    }
  return FL_SUCCESS;
}

// ---- Dirichlet forcing of one scalar, and what it hands to the fluid ------------------------------------------------------------------------

extern "C" int fl_ibm_scalar_force(fl_ibm *m, int npass, const double *target_dev, const int32_t *body_dev, int nbody, const double *value, const double *dV_dev, double *phi_dev, double *Q_dev)
{
  if (!m) return FL_ERR_ARG_NULL;
  fl_poisson   *h     = m->gp;
  hipStream_t   s     = h->stream;
  const bool    split = h->multi || ibm_split(h);
  const int64_t L     = m->owned ? m->Lo : m->P.L;
  const bool    null_arg = !phi_dev || (L > 0 && !dV_dev);
  const bool    range_ok = npass >= 1 && npass <= 16 && nbody >= 1 && nbody <= FORCE_MAXBODY;
  const bool    wrong    = (target_dev && value) || (L > 0 && !target_dev && !value);
  FL_HIP(hipSetDevice(h->device));
  if (m->owned && split) {  // collective: every rank leaves with the same error, or none does
    double v[3] = {null_arg ? 1. : 0., range_ok ? 0. : 1., wrong ? 1. : 0.};
    FL_CHK(ibm_vote(h, v, 3));
    if (v[0] > 0.) return FL_ERR_ARG_NULL;
    if (v[1] > 0.) return FL_ERR_ARG_OUTOFRANGE;
    if (v[2] > 0.) return FL_ERR_ARG_WRONG;
  } else {
    if (null_arg) return FL_ERR_ARG_NULL;
    if (!range_ok) return FL_ERR_ARG_OUTOFRANGE;
    if (wrong) return FL_ERR_ARG_WRONG;
  }
  ScalarTarget V;
  for (int b = 0; b < FORCE_MAXBODY; ++b) V.value[b] = (value && b < nbody) ? value[b] : 0.;
  const int32_t *body = value ? body_dev : nullptr;
  if (L > 0) FL_CHK(ibm_reserve(h, &m->sq, &m->sqcap, L));
  if (L > 0 && split) FL_CHK(ibm_reserve(h, &m->sphi, &m->sphicap, L));
  const unsigned nbq = (unsigned)((L + 255) / 256);
  for (int k = 0; k < npass; ++k) {
    if (!split) {
      // one rank: every marker's support is here (P.L = L, an owned set holds no ghost) -- the defect in the interpolation's launch
      if (L > 0) hipLaunchKernelGGL(k_ibm_scalar_defect, dim3((unsigned)((L + 3) / 4)), dim3(256), 0, s, m->P, m->i0, m->w, phi_dev, target_dev, body, V, k == 0, m->sq, Q_dev);
      if (m->nactive > 0) hipLaunchKernelGGL(k_ibm_spread<1>, dim3(m->nactive), dim3(256), 0, s, m->P, m->i0, m->w, m->off, m->list, m->active, 1, h->ncell, m->sq, dV_dev, phi_dev);
      FL_HIP(hipGetLastError());
    } else if (m->owned) {
      FL_CHK(ibm_interp_owned(m, 1, phi_dev, m->sphi));  // own + ghost markers, the ghosts' partial sums back to their owners
      if (L > 0) hipLaunchKernelGGL(k_ibm_scalar_q, dim3(nbq), dim3(256), 0, s, L, m->sphi, target_dev, body, V, k == 0, m->sq, Q_dev);
      FL_HIP(hipGetLastError());
      FL_CHK(ibm_spread_owned(m, 1, m->sq, dV_dev, phi_dev, true));
    } else {
      hipLaunchKernelGGL(k_ibm_interp, dim3((unsigned)((L + 3) / 4)), dim3(256), 0, s, m->P, m->i0, m->w, 1, h->ncell, phi_dev, m->sphi);
      FL_HIP(hipGetLastError());
      if (h->comm.kind == Comm::NONE) return FL_ERR_ARG_WRONGSTATE;
      FL_CHK(h->comm.allreduce(s, m->sphi, (int)L));  // where fl_ibm_interp has it
      hipLaunchKernelGGL(k_ibm_scalar_q, dim3(nbq), dim3(256), 0, s, L, m->sphi, target_dev, body, V, k == 0, m->sq, Q_dev);
      if (m->nactive > 0) hipLaunchKernelGGL(k_ibm_spread<1>, dim3(m->nactive), dim3(256), 0, s, m->P, m->i0, m->w, m->off, m->list, m->active, 1, h->ncell, m->sq, dV_dev, phi_dev);
      FL_HIP(hipGetLastError());
    }
  }
  return FL_SUCCESS;
}

// The sum is fl_ibm_force's, on F = (Q, 0, 0): its force group then holds the terms Q_l dV_l and nothing else (a zero term changes neither the
// maximum nor an integer sum), so the split, the bound, the NaN rule, the votes and the collectives are that call's own.  The torque group it
// also forms is not used.
extern "C" int fl_ibm_scalar_rate(fl_ibm *m, const double *Q_dev, const double *dV_dev, const int32_t *body_dev, int nbody, double *rate)
{
  if (!m) return FL_ERR_ARG_NULL;
  fl_poisson   *h = m->gp;
  const int64_t L = m->owned ? m->Lo : m->P.L;
  FL_HIP(hipSetDevice(h->device));
  const double *F = nullptr;
  if (L > 0 && Q_dev) {
    FL_CHK(ibm_reserve(h, &m->sf3, &m->sf3cap, 3 * L));
    FL_HIP(hipMemcpyAsync(m->sf3, Q_dev, sizeof(double) * (size_t)L, hipMemcpyDeviceToDevice, h->stream));
    FL_HIP(hipMemsetAsync(m->sf3 + L, 0, sizeof(double) * 2 * (size_t)L, h->stream));
    F = m->sf3;
  }
  const int           nb = std::min(std::max(nbody, 1), FORCE_MAXBODY);
  std::vector<double> about(3 * (size_t)nb, 0.), force(3 * (size_t)nb, 0.);
  // nbody out of range: fl_ibm_force says so (and votes it) before it reads or writes an array sized by it
  const int rc = fl_ibm_force(m, F, dV_dev, body_dev, nbody, about.data(), rate ? force.data() : nullptr, nullptr);
  if (rc) return rc;
  for (int b = 0; b < nbody; ++b) rate[b] = force[3 * (size_t)b];
  return FL_SUCCESS;
}

extern "C" int fl_ibm_destroy(fl_ibm *m)
{
  if (!m) return FL_SUCCESS;
  if (m->gp) (void)hipStreamSynchronize(m->gp->stream);
  for (void *p : {(void *)m->X, (void *)m->Y, (void *)m->Z, (void *)m->w, (void *)m->i0, (void *)m->cnt, (void *)m->off, (void *)m->list, (void *)m->scratch, (void *)m->active, (void *)m->nact_dev, (void *)m->xcg[0],
                  (void *)m->xcg[1], (void *)m->xcg[2], (void *)m->gid_own, (void *)m->gid, (void *)m->mask, (void *)m->sendlist, (void *)m->cstart, (void *)m->clist, (void *)m->sbuf, (void *)m->rbuf, (void *)m->Ui,
                  (void *)m->Fi, (void *)m->cbuf, (void *)m->dest, (void *)m->bstay, (void *)m->boff, (void *)m->mcnt, (void *)m->gidtmp, (void *)m->stay, (void *)m->arr, (void *)m->mpos, (void *)m->attr,
                  (void *)m->attrtmp, (void *)m->nbuf, (void *)m->fws, (void *)m->ftick, (void *)m->sq, (void *)m->sphi, (void *)m->sf3})
    if (p) (void)hipFree(p);
  delete m;
  return FL_SUCCESS;
}
