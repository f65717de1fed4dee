// fl_ibm_handle.h -- the fl_ibm handle (its device memory: DevBuf, fl_devbuf.h) and the host functions that cross between fl_ibm.hip (the marker
// set), fl_ibm_owner.hip (owner-rank markers, migration) and fl_ibm_body.hip (per-body sums, the scalar on the markers).  Every __global__ function
// lives in exactly one of the three; a unit that needs another's kernel calls one of the launchers declared below.
#pragma once
#include "fl_devbuf.h"
#include "fl_handle.h"
#include "fl_ibm_device.h"
#include "fl_ibm_plan.h"

#pragma GCC visibility push(hidden)  // internal to the library: its dynamic symbols stay the C-ABI's

namespace fl {

struct RouteP {
  int peer_lo[3], peer_hi[3];  // ibm_plan_peers'
};

struct DestP {
  int peer_lo[3], peer_hi[3];      // RouteP's
  int lo_beg[3], lo_end[3];        // GLOBAL cells [beg, end) of the block behind the low end of this one along the axis (the periodic wrap included)
  int hi_beg[3], hi_end[3];        // ... behind the high end
};

}  // namespace fl

struct fl_ibm {
  // ---- fl_ibm.hip: the marker set, its weights and its bins
  fl_poisson     *gp = nullptr;        // borrowed: grid, device, stream
  IbmP            P;                   // the set as a kernel sees it; P.L = markers held (an owner-rank set: Lo + Lg, own markers first, then the ghosts
                                       // grouped by ascending offset code)
  DevBuf<double>  X, Y, Z, w;          // per-marker group: positions, the 12 1-D weights
  DevBuf<int>     i0, list, scratch;   // per-marker group: first support cells; the bins and the scratch of their sort (listcap entries each)
  DevBuf<int64_t> gid;                 // per-marker group, owner-rank sets: the caller's numbers of own + ghost markers (sort key of the bins)
  int64_t         cap = -1;            // markers the per-marker group holds (ibm_alloc_markers)
  int             listcap = 0;
  DevBuf<int>     cnt, off, active, nact_dev;  // per tile: bin sizes, bin starts, the tiles with a non-empty bin and their number
  int             ntiles = 0, nactive = 0;
  DevBuf<double>  xcg[3];              // the extended global centre arrays of the stretched axes (P.xcg points one past their start)
  // ---- fl_ibm_owner.hip: owner-rank markers (fl_ibm_create_owned)
  bool            owned = false, has_gid = false;
  int64_t         Lo = 0, Lg = 0;      // own markers, ghost markers held
  int             ncopy = 0;           // copies of own markers held by other ranks
  RouteP          R;
  int             peer[27], scnt[27], soff[27], gcnt[27], goff[27];  // per offset code: rank behind it (-1 none), copies sent / ghosts held and where they start
  DevBuf<int64_t> gid_own;             // the caller's numbers of the own markers (kept for update)
  DevBuf<int>     mask;                // k_ibm_route's result
  DevBuf<int>     sendlist, cstart, clist;  // the own marker of every copy; per own marker its copies [cstart[l], cstart[l+1]) in clist
  DevBuf<double>  sbuf, rbuf;          // message records out / in
  DevBuf<double>  Ui, Fi;              // U and (F, dV) of own + ghost markers
  DevBuf<double>  cbuf;                // the count exchange: 27 counts out, 27 in
  // ---- fl_ibm_owner.hip: migration (fl_ibm_migrate)
  bool            nbr_known = false;   // D holds the neighbours' cell ranges (exchanged once per set)
  DestP           D;
  DevBuf<double>  nbuf;                // that exchange: (lo, n) of this block, then of the block behind every offset code
  DevBuf<int>     dest, bstay, boff;   // per own marker its destination; per block of 256 the stayers and where they start
  DevBuf<int>     mcnt;                // MIG_NCNT counts + 28 offsets + 27 cursors
  DevBuf<double>  stay, arr, mpos;     // stayers, ranked arrivals, the merged positions
  DevBuf<int64_t> gidtmp;              // the merged numbers: swapped with gid_own
  DevBuf<double>  attr, attrtmp;       // the attributes of the last call (fl_ibm_owned_fetch) and the merged ones: swapped
  int             nattr = 0;
  // ---- fl_ibm_body.hip: per-body sums, the scalar on the markers
  DevBuf<double>   fws;                // fl_ibm_force: workspace (FW_END doubles)
  DevBuf<unsigned> ftick;              // ... and its two arrival counters (16 bytes, zeroed before every call)
  DevBuf<double>   sq, sphi;           // fl_ibm_scalar_force: q and the complete Phi of a pass (one value per marker of the set)
  DevBuf<double>   sf3;                // fl_ibm_scalar_rate: (Q, 0, 0) for the sum
};

// ---- shared by the three units

inline bool ibm_split(const fl_poisson *h) { return h->dec.ranks[0] * h->dec.ranks[1] * h->dec.ranks[2] > 1; }

// sum of n <= 8 flags over the ranks: every rank takes the same way out of a collective call
inline int ibm_vote(fl_poisson *h, double *v, int n)
{
  if (!ibm_split(h)) return 0;
  if (h->comm.kind == Comm::NONE) return FL_ERR_ARG_WRONGSTATE;
  return fl_poisson_allreduce_sum(h, v, n);
}

// what fl_ibm_create and fl_ibm_owned_select ask of the delta function and of the number of markers
inline int ibm_check_kind_count(int kind, int64_t L)
{
  if (kind != FL_DELTA_PESKIN4 && kind != FL_DELTA_ROMA3) return FL_ERR_ARG_OUTOFRANGE;
  if (L < 1 || L > (int64_t)1 << 27) return FL_ERR_ARG_OUTOFRANGE;
  return 0;
}

// n positions from one set of three device arrays to another in stream order; a destination that is absent is skipped
inline int ibm_copy_xyz(hipStream_t s, size_t n, double *X, double *Y, double *Z, const double *Xs, const double *Ys, const double *Zs)
{
  if (X) FL_HIP(hipMemcpyAsync(X, Xs, sizeof(double) * n, hipMemcpyDeviceToDevice, s));
  if (Y) FL_HIP(hipMemcpyAsync(Y, Ys, sizeof(double) * n, hipMemcpyDeviceToDevice, s));
  if (Z) FL_HIP(hipMemcpyAsync(Z, Zs, sizeof(double) * n, hipMemcpyDeviceToDevice, s));
  return 0;
}

// fl_ibm.hip
int  ibm_geometry(fl_poisson *h, int kind, IbmP &P, DevBuf<double> xcg[3]);
int  ibm_new(fl_poisson *h, int kind, bool owned, fl_ibm **out);
int  ibm_alloc_markers(fl_ibm *m, int64_t L);
int  ibm_rebin(fl_ibm *m);
// launches on the handle's stream; the caller asks hipGetLastError where it always has
void ibm_launch_interp(fl_ibm *m, int64_t L, int ncomp, const double *u, double *U);                           // k_ibm_interp, one wavefront per marker
void ibm_launch_spread(fl_ibm *m, int ncomp, const double *F, const double *dV, double *f, bool one = false);  // k_ibm_spread<3>, or <1> with ncomp = 1 (one); nothing without an occupied bin
void ibm_launch_scan(hipStream_t s, const int *cnt, int *off, int n);                                          // k_ibm_scan
// fl_ibm_owner.hip
int ibm_route(fl_ibm *m, int64_t Lo, const double *X, const double *Y, const double *Z, const int64_t *gid_new, bool first);
int ibm_interp_owned(fl_ibm *m, int ncomp, const double *u, double *U);
int ibm_spread_owned(fl_ibm *m, int ncomp, const double *F, const double *dV, double *f, bool one = false);

#pragma GCC visibility pop
