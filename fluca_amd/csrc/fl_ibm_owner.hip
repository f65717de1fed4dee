// fl_ibm_owner.hip -- owner-rank markers (fl_ibm.hip's header): routing own markers to the neighbours that hold ghost copies,
// interpolation and spreading over own + ghost markers, and migration of a marker to the rank its owner cell has moved to.  The rule that orders the
// messages of every exchange here is ibm_plan_msgs' (fl_ibm_plan.h).
#include "fl_ibm_handle.h"

namespace fl {

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

// ---- migration (fl_ibm_migrate) -----------------------------------------------------------------------------------------------------------
// Every record and every staging array below is made of doubles: position, the marker number (< 2^27: exact) and up to 8 attributes.
constexpr int MIG_NCNT = 32;  // cnt[0..26] markers per destination offset (13: stay), cnt[27] out of reach, cnt[28] numbers not ascending, cnt[29] spare

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

}  // namespace fl

// ---- routing (set-up time: host waits as in ibm_rebin) --------------------------------------------------------------------------------------

// the masks of k_ibm_route for L markers at (X, Y, Z), on the host
static int ibm_masks(fl_ibm *m, const RouteP &R, int64_t L, const double *X, const double *Y, const double *Z, std::vector<int> &host)
{
  fl_poisson *h = m->gp;
  host.assign((size_t)L, 0);
  if (L == 0) return 0;
  FL_CHK(m->mask.reserve(h, L));
  IbmP P = m->P;
  P.L    = L;
  hipLaunchKernelGGL(k_ibm_route, dim3((unsigned)((L + 255) / 256)), dim3(256), 0, h->stream, P, R, X, Y, Z, m->mask);
  FL_HIP(hipGetLastError());
  FL_HIP(hipMemcpyAsync(host.data(), m->mask, sizeof(int) * (size_t)L, hipMemcpyDeviceToHost, h->stream));
  FL_HIP(hipStreamSynchronize(h->stream));
  return 0;
}

// One exchange between owners and ghost holders and its messages.  to_ghosts: the owners send (spread, positions), else the ghost holders do
// (interp).  per = doubles per copy.  Empty messages are left out: both sides know every count.
static int ibm_exchange(fl_ibm *m, bool to_ghosts, int per)
{
  std::vector<Msg> msgs;
  if (to_ghosts) ibm_plan_msgs(m->peer, m->scnt, m->soff, m->gcnt, m->goff, per, m->sbuf, m->rbuf, false, msgs);
  else ibm_plan_msgs(m->peer, m->gcnt, m->goff, m->scnt, m->soff, per, m->sbuf, m->rbuf, false, msgs);
  return m->gp->comm.exchange(m->gp->stream, msgs);
}

// Every rank tells the rank behind each offset how many records it is about to send there: cnt[27] out, got[27] back (0 where no rank is), one double
// per message, through cbuf (27 counts out, 27 in).  The host waits for the counts.
static int ibm_exchange_counts(fl_ibm *m, const int cnt[27], int got[27])
{
  fl_poisson *h = m->gp;
  hipStream_t s = h->stream;
  if (m->cbuf.once(h, 54, true)) return FL_ERR_MEM;
  double hc[54];
  int    one[27], out[27], in[27];
  for (int code = 0; code < 27; ++code) {
    hc[code] = (double)cnt[code], hc[27 + code] = 0.;
    one[code] = 1, out[code] = code, in[code] = 27 + code;
  }
  FL_HIP(hipMemcpyAsync(m->cbuf, hc, sizeof(hc), hipMemcpyHostToDevice, s));
  std::vector<Msg> msgs;
  ibm_plan_msgs(m->peer, one, out, one, in, 1, m->cbuf, m->cbuf, true, msgs);
  FL_CHK(h->comm.exchange(s, msgs));
  FL_HIP(hipMemcpyAsync(hc, m->cbuf, sizeof(hc), hipMemcpyDeviceToHost, s));
  FL_HIP(hipStreamSynchronize(s));
  for (int code = 0; code < 27; ++code) got[code] = m->peer[code] >= 0 ? (int)hc[27 + code] : 0;
  return 0;
}

// own markers (Lo of them, the caller's device arrays) -> ghost copies on the neighbours, marker arrays of own + ghost, bins.  Collective.
int ibm_route(fl_ibm *m, int64_t Lo, const double *X, const double *Y, const double *Z, const int64_t *gid_new, bool first)
{
  fl_poisson *h = m->gp;
  hipStream_t s = h->stream;
  const IbmP &P = m->P;
  // which offsets have a rank behind them
  RouteP R;
  int    peer[27];
  ibm_plan_peers(&h->dec, P.periodic, R.peer_lo, R.peer_hi, peer);
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
  m->sendlist.release(h), m->cstart.release(h), m->clist.release(h);  // the group is released, then allocated (ibm_alloc_markers)
  if (m->sendlist.exact(h, ncopy, false) || m->cstart.exact(h, Lo + 1, false) || m->clist.exact(h, ncopy, false)) return FL_ERR_MEM;
  if (ncopy) FL_HIP(hipMemcpyAsync(m->sendlist, sendlist.data(), sizeof(int) * (size_t)ncopy, hipMemcpyHostToDevice, s));
  if (ncopy) FL_HIP(hipMemcpyAsync(m->clist, clist.data(), sizeof(int) * (size_t)ncopy, hipMemcpyHostToDevice, s));
  FL_HIP(hipMemcpyAsync(m->cstart, cstart.data(), sizeof(int) * ((size_t)Lo + 1), hipMemcpyHostToDevice, s));
  if (first && m->has_gid && Lo > 0) {
    if (m->gid_own.exact(h, Lo, false)) return FL_ERR_MEM;
    FL_HIP(hipMemcpyAsync(m->gid_own, gid_new, sizeof(int64_t) * (size_t)Lo, hipMemcpyDeviceToDevice, s));
  }
  // the counts of the copies, one double per offset that has a rank behind it
  int64_t Lg = 0;
  if (ibm_split(h)) FL_CHK(ibm_exchange_counts(m, m->scnt, m->gcnt));  // (its host wait: the sendlist vectors above are still alive here)
  else FL_HIP(hipStreamSynchronize(s));
  for (int code = 0; code < 27; ++code) m->goff[code] = (int)Lg, Lg += m->gcnt[code];
  m->Lg             = Lg;
  const int64_t Lt = Lo + Lg;
  if (Lt > (int64_t)1 << 27) return FL_ERR_ARG_OUTOFRANGE;
  m->P.L = Lt;
  FL_CHK(ibm_alloc_markers(m, Lt));
  if (Lo > 0) {
    FL_CHK(ibm_copy_xyz(s, (size_t)Lo, m->X, m->Y, m->Z, X, Y, Z));
    if (m->has_gid) FL_HIP(hipMemcpyAsync(m->gid, m->gid_own, sizeof(int64_t) * (size_t)Lo, hipMemcpyDeviceToDevice, s));
  }
  // positions (and numbers) of the copies
  if (ncopy > 0 || Lg > 0) {
    FL_CHK(m->sbuf.reserve(h, 4 * (int64_t)ncopy));
    FL_CHK(m->rbuf.reserve(h, 4 * Lg));
    if (ncopy > 0) hipLaunchKernelGGL(k_ibm_pack_pos, dim3((ncopy + 255) / 256), dim3(256), 0, s, ncopy, m->sendlist, m->X, m->Y, m->Z, (const int64_t *)(m->has_gid ? m->gid.p : nullptr), m->sbuf);
    FL_CHK(ibm_exchange(m, true, 4));
    if (Lg > 0) hipLaunchKernelGGL(k_ibm_unpack_pos, dim3((unsigned)((Lg + 255) / 256)), dim3(256), 0, s, (int)Lg, Lo, m->rbuf, m->X, m->Y, m->Z, m->has_gid ? m->gid.p : nullptr);
    FL_HIP(hipGetLastError());
  }
  return ibm_rebin(m);
}

extern "C" int fl_ibm_owned_select(fl_poisson *h, int kind, int64_t L, const double *X, const double *Y, const double *Z, int64_t *idx_out_dev, int64_t *count_out)
{
  if (!h || !X || !Y || !Z || !idx_out_dev || !count_out) return FL_ERR_ARG_NULL;
  FL_CHK(ibm_check_kind_count(kind, L));
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

// ---- per call (stream-ordered; the host waits only where the host transport itself does) ---------------------------------------------------

int ibm_interp_owned(fl_ibm *m, int ncomp, const double *u, double *U)
{
  fl_poisson   *h  = m->gp;
  hipStream_t   s  = h->stream;
  const int64_t Lo = m->Lo, Lg = m->Lg, Lt = Lo + Lg;
  if (Lo > 0 && !U) return FL_ERR_ARG_NULL;
  if (Lt == 0) return FL_SUCCESS;
  FL_CHK(m->Ui.reserve(h, (int64_t)ncomp * Lt));
  FL_CHK(m->sbuf.reserve(h, (int64_t)ncomp * Lg));
  FL_CHK(m->rbuf.reserve(h, (int64_t)ncomp * m->ncopy));
  ibm_launch_interp(m, Lt, ncomp, u, m->Ui);
  if (Lg > 0) hipLaunchKernelGGL(k_ibm_pack_U, dim3((unsigned)((Lg + 255) / 256)), dim3(256), 0, s, (int)Lg, Lo, Lt, ncomp, m->Ui, m->sbuf);
  FL_HIP(hipGetLastError());
  if (Lg > 0 || m->ncopy > 0) FL_CHK(ibm_exchange(m, false, ncomp));
  if (Lo > 0) hipLaunchKernelGGL(k_ibm_collect_U, dim3((unsigned)((Lo + 255) / 256)), dim3(256), 0, s, Lo, Lt, ncomp, m->Ui, m->cstart, m->clist, m->rbuf, U);
  FL_HIP(hipGetLastError());
  return FL_SUCCESS;
}

// one: the one-component kernel of the scalar forcing (ncomp = 1), else fl_ibm_spread's
int ibm_spread_owned(fl_ibm *m, int ncomp, const double *F, const double *dV, double *f, bool one)
{
  fl_poisson   *h  = m->gp;
  hipStream_t   s  = h->stream;
  const int64_t Lo = m->Lo, Lg = m->Lg, Lt = Lo + Lg;
  if (Lo > 0 && (!F || !dV)) return FL_ERR_ARG_NULL;
  if (Lt == 0) return FL_SUCCESS;
  const int per = ncomp + 1;
  FL_CHK(m->Fi.reserve(h, (int64_t)per * Lt));
  FL_CHK(m->sbuf.reserve(h, (int64_t)per * m->ncopy));
  FL_CHK(m->rbuf.reserve(h, (int64_t)per * Lg));
  if (m->ncopy > 0) hipLaunchKernelGGL(k_ibm_pack_F, dim3((m->ncopy + 255) / 256), dim3(256), 0, s, m->ncopy, Lo, ncomp, m->sendlist, F, dV, m->sbuf);
  FL_HIP(hipGetLastError());
  if (Lg > 0 || m->ncopy > 0) FL_CHK(ibm_exchange(m, true, per));
  double *Fi = m->Fi, *dVi = m->Fi + (int64_t)ncomp * Lt;
  hipLaunchKernelGGL(k_ibm_stage_F, dim3((unsigned)((Lt + 255) / 256)), dim3(256), 0, s, Lo, Lt, ncomp, F, dV, m->rbuf, Fi, dVi);
  ibm_launch_spread(m, ncomp, Fi, dVi, f, one);
  FL_HIP(hipGetLastError());
  return FL_SUCCESS;
}

// ---- migration ------------------------------------------------------------------------------------------------------------------------------

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
  if (m->nbuf.once(h, 6 * 28, true)) return FL_ERR_MEM;
  double hb[6 * 28] = {0.};
  for (int d = 0; d < 3; ++d) hb[d] = (double)P.lo[d], hb[3 + d] = (double)P.n[d];
  FL_HIP(hipMemcpyAsync(m->nbuf, hb, sizeof(double) * 6, hipMemcpyHostToDevice, s));
  // one record of 6 doubles: sent from slot 0 under every face code, the neighbour's received in slot 1 + code
  int one[27], zero[27], slot[27];
  for (int code = 0; code < 27; ++code) one[code] = 1, zero[code] = 0, slot[code] = 1 + code;
  std::vector<Msg> msgs;
  ibm_plan_msgs(m->peer, one, zero, one, slot, 6, m->nbuf, m->nbuf, true, msgs, IBM_FACE_CODES);
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
  if (m->mcnt.once(h, MIG_NCNT + 28 + 27, true)) return FL_ERR_MEM;
  int hc[MIG_NCNT] = {0};
  if (Lo > 0) {
    FL_CHK(m->dest.reserve(h, Lo));
    FL_CHK(m->bstay.reserve(h, nb + 1));
    FL_CHK(m->boff.reserve(h, nb + 1));
    FL_HIP(hipMemsetAsync(m->mcnt, 0, sizeof(int) * (MIG_NCNT + 28 + 27), s));
    IbmP P = m->P;
    P.L    = Lo;
    hipLaunchKernelGGL(k_ibm_dest, dim3(nb), dim3(256), 0, s, P, m->D, X, Y, Z, (const int64_t *)m->gid_own, m->dest, m->mcnt, m->bstay);
    FL_HIP(hipGetLastError());
    FL_HIP(hipMemcpyAsync(hc, m->mcnt, sizeof(hc), hipMemcpyDeviceToHost, s));
    FL_HIP(hipStreamSynchronize(s));
  }
  // 2. the votes, then the counts to and from the neighbours
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
  if (ibm_split(h)) FL_CHK(ibm_exchange_counts(m, lcnt, acnt));
  for (int code = 0; code < 27; ++code) aoff[code] = (int)A, A += acnt[code];
  aoff[27]          = (int)A;
  const int64_t Ls = Lo - nleave, Ln = Ls + A;
  if (Ln > (int64_t)1 << 27) return FL_ERR_ARG_OUTOFRANGE;
  m->nattr = nattr;
  if (nleave == 0 && A == 0) {
    // nothing crosses a face of this block: the list stays as it is, only the attributes are kept for fl_ibm_owned_fetch
    if (nattr > 0 && Lo > 0) {
      FL_CHK(m->attr.reserve(h, (int64_t)nattr * Lo));
      FL_HIP(hipMemcpyAsync(m->attr, attr_dev, sizeof(double) * (size_t)nattr * (size_t)Lo, hipMemcpyDeviceToDevice, s));
    }
    *L_local_new = Lo;
    moved[0] = moved[1] = 0;
    return ibm_route(m, Lo, X, Y, Z, nullptr, false);
  }
  const int per = 4 + nattr;
  FL_CHK(m->sbuf.reserve(h, per * nleave));
  FL_CHK(m->rbuf.reserve(h, per * A));
  FL_CHK(m->stay.reserve(h, per * Ls));
  FL_CHK(m->arr.reserve(h, per * A));
  FL_CHK(m->mpos.reserve(h, 3 * Ln));
  FL_CHK(m->gidtmp.reserve(h, Ln));
  FL_CHK(m->attrtmp.reserve(h, (int64_t)nattr * Ln));
  // 3. + 4. stayers compacted in order, leavers packed by offset
  if (Lo > 0) {
    int *leaveoff = m->mcnt + MIG_NCNT, *cursor = m->mcnt + MIG_NCNT + 28;
    FL_HIP(hipMemcpyAsync(leaveoff, loff, sizeof(loff), hipMemcpyHostToDevice, s));
    ibm_launch_scan(s, m->bstay, m->boff, nb);
    hipLaunchKernelGGL(k_ibm_split, dim3(nb), dim3(256), 0, s, Lo, Ls, nattr, m->dest, m->boff, leaveoff, cursor, X, Y, Z, (const int64_t *)m->gid_own, attr_dev, m->stay, m->sbuf);
    FL_HIP(hipGetLastError());
  }
  // 5. one exchange: a message per offset that carries a record
  {
    std::vector<Msg> msgs;
    ibm_plan_msgs(m->peer, lcnt, loff, acnt, aoff, per, m->sbuf, m->rbuf, false, msgs);
    FL_CHK(h->comm.exchange(s, msgs));
  }
  // 6. + 7. arrivals by number, then both ascending lists into one
  if (A > 0) hipLaunchKernelGGL(k_ibm_rank_arrivals, dim3((unsigned)((A + 255) / 256)), dim3(256), 0, s, (int)A, per, m->rbuf, m->arr);
  if (Ln > 0) hipLaunchKernelGGL(k_ibm_merge, dim3((unsigned)((Ln + 255) / 256)), dim3(256), 0, s, Ls, A, nattr, m->stay, m->arr, m->mpos, m->gidtmp, m->attrtmp);
  FL_HIP(hipGetLastError());
  m->gid_own.swap(m->gidtmp);
  m->attr.swap(m->attrtmp);
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
  FL_CHK(ibm_copy_xyz(s, n, X, Y, Z, m->X, m->Y, m->Z));
  if (gid) FL_HIP(hipMemcpyAsync(gid, m->gid_own, sizeof(int64_t) * n, hipMemcpyDeviceToDevice, s));
  if (nattr > 0) FL_HIP(hipMemcpyAsync(attr_out, m->attr, sizeof(double) * n * (size_t)nattr, hipMemcpyDeviceToDevice, s));
  return FL_SUCCESS;
}
