// fl_ibm_device.h -- what the immersed-boundary kernels of more than one translation unit share (fl_ibm.hip, fl_ibm_owner.hip, fl_ibm_body.hip): the
// marker set as a kernel sees it, the delta functions, a marker's continuous cell-centre index and its support cells.  The specification is in
// fl_ibm.hip's header.
#pragma once
#include "fl_internal.h"

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

}  // namespace fl
