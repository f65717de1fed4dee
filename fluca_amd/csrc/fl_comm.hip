// fl_comm.hip -- the transports of a handle's communicator (RCCL Send / Recv / AllReduce; host-staged callbacks; the one-shot all-reduce
// through peer-mapped mailboxes with its kernel) behind struct Comm (fl_handle.h), and their C-ABI.
#include <dlfcn.h>
#include <rccl/rccl.h>

#include <atomic>
#include <ctime>
#include <mutex>

#include "fl_handle.h"

namespace fl {
namespace {

struct Rccl {
  void *lib = nullptr;
  decltype(&ncclGetUniqueId)    GetUniqueId    = nullptr;
  decltype(&ncclCommInitRank)   CommInitRank   = nullptr;
  decltype(&ncclCommDestroy)    CommDestroy    = nullptr;
  decltype(&ncclSend)           Send           = nullptr;
  decltype(&ncclRecv)           Recv           = nullptr;
  decltype(&ncclAllReduce)      AllReduce      = nullptr;
  decltype(&ncclGroupStart)     GroupStart     = nullptr;
  decltype(&ncclGroupEnd)       GroupEnd       = nullptr;
  decltype(&ncclGetErrorString) GetErrorString = nullptr;
  decltype(&ncclCommCount)      CommCount      = nullptr;
  decltype(&ncclCommUserRank)   CommUserRank   = nullptr;
  std::mutex mu;  // handles of several host threads may reach their first RCCL call together
  int        load()
  {
    std::lock_guard<std::mutex> lock(mu);
    if (lib) return 0;
    // the soname: inside a process that already loaded torch this resolves to the very RCCL torch.distributed uses
    void *l = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!l) l = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
    if (!l) {
      std::fprintf(stderr, "[flucahip] cannot dlopen librccl: %s\n", dlerror());
      return FL_ERR_LIB;
    }
#define FL_SYM(n)                                                \
  n = (decltype(n))dlsym(l, "nccl" #n);                          \
  if (!n) {                                                      \
    std::fprintf(stderr, "[flucahip] librccl lacks nccl" #n "\n"); \
    return FL_ERR_LIB;                                           \
  }
    FL_SYM(GetUniqueId) FL_SYM(CommInitRank) FL_SYM(CommDestroy) FL_SYM(Send) FL_SYM(Recv) FL_SYM(AllReduce) FL_SYM(GroupStart) FL_SYM(GroupEnd) FL_SYM(GetErrorString) FL_SYM(CommCount) FL_SYM(CommUserRank)
#undef FL_SYM
    lib = l;  // last: a reader that sees lib != nullptr sees every symbol
    return 0;
  }
};
Rccl g_rccl;

#define FL_NCCL(call)                                                                                              \
  do {                                                                                                             \
    ncclResult_t r_ = (call);                                                                                      \
    if (r_ != ncclSuccess) {                                                                                       \
      std::fprintf(stderr, "[flucahip] %s:%d %s -> %s\n", __FILE__, __LINE__, #call, g_rccl.GetErrorString(r_)); \
      return FL_ERR_LIB;                                                                                           \
    }                                                                                                              \
  } while (0)

}  // namespace

int Comm::exchange(hipStream_t st, const std::vector<Msg> &m)
{
  if (m.empty()) return 0;
  if (kind == RCCL) {
    FL_NCCL(g_rccl.GroupStart());
    // a failing Send / Recv must not leave the communicator inside an open group: remember the error, close the group, report
    ncclResult_t bad = ncclSuccess;
    for (const Msg &x : m) {
      if (bad == ncclSuccess && x.send) bad = g_rccl.Send(x.send, (size_t)x.count, ncclDouble, x.peer, nccl, st);
      if (bad == ncclSuccess && x.recv) bad = g_rccl.Recv(x.recv, (size_t)x.count, ncclDouble, x.peer, nccl, st);
    }
    const ncclResult_t end = g_rccl.GroupEnd();
    if (bad != ncclSuccess || end != ncclSuccess) {
      std::fprintf(stderr, "[flucahip] halo exchange over RCCL failed: %s\n", g_rccl.GetErrorString(bad != ncclSuccess ? bad : end));
      return FL_ERR_LIB;
    }
    return 0;
  }
  if (kind == HOST) {
    const int n = (int)m.size();
    if (knob(K_comm_trace) != 0) {
      static std::atomic<long> seq{0};
      struct timespec ts;
      clock_gettime(CLOCK_MONOTONIC, &ts);
      std::fprintf(stderr, "[%.3f comm r%d #%ld] exchange %d msgs:", ts.tv_sec % 1000 + 1e-9 * ts.tv_nsec, rank, seq.fetch_add(1), n);
      for (const Msg &x : m) std::fprintf(stderr, " (peer %d stag %d rtag %d n %lld%s%s)", x.peer, x.sendtag, x.recvtag, (long long)x.count, x.send ? " S" : "", x.recv ? " R" : "");
      std::fprintf(stderr, "\n");
      std::fflush(stderr);
    }
    if ((int)hsend.size() < n) {
      hsend.resize(n, nullptr);
      hrecv.resize(n, nullptr);
      hcap.resize(n, 0);
    }
    std::vector<int>     peer(n), stag(n), rtag(n);
    std::vector<void *>  sp(n), rp(n);
    std::vector<int64_t> nb(n);
    for (int a = 0; a < n; ++a) {
      if (hcap[a] < m[a].count) {
        if (hsend[a]) (void)hipHostFree(hsend[a]);
        if (hrecv[a]) (void)hipHostFree(hrecv[a]);
        FL_HIP(hipHostMalloc((void **)&hsend[a], sizeof(double) * m[a].count));
        FL_HIP(hipHostMalloc((void **)&hrecv[a], sizeof(double) * m[a].count));
        hcap[a] = m[a].count;
      }
      if (m[a].send) FL_HIP(hipMemcpyAsync(hsend[a], m[a].send, sizeof(double) * m[a].count, hipMemcpyDeviceToHost, st));
      peer[a] = m[a].peer;
      stag[a] = m[a].sendtag;
      rtag[a] = m[a].recvtag;
      sp[a]   = m[a].send ? hsend[a] : nullptr;
      rp[a]   = m[a].recv ? hrecv[a] : nullptr;
      nb[a]   = (int64_t)sizeof(double) * m[a].count;
    }
    FL_HIP(hipStreamSynchronize(st));
    if (xchg(ctx, n, peer.data(), stag.data(), rtag.data(), sp.data(), rp.data(), nb.data()) != 0) return FL_ERR_LIB;
    for (int a = 0; a < n; ++a)
      if (m[a].recv) FL_HIP(hipMemcpyAsync(m[a].recv, hrecv[a], sizeof(double) * m[a].count, hipMemcpyHostToDevice, st));
    return 0;
  }
  return FL_ERR_ARG_WRONGSTATE;
}


int Comm::allreduce(hipStream_t st, double *dev, int n)
{
  if (nranks == 1 && !loopback) return 0;
  if (oneshot_ready && n <= NSLOT && knob(K_allreduce) == 1) {
    launch_oneshot_allreduce(st, peers_dev, rank, nranks, ++oneshot_calls, dev, n);
    return 0;
  }
  if (kind == RCCL) {
    FL_NCCL(g_rccl.AllReduce(dev, dev, (size_t)n, ncclDouble, ncclSum, nccl, st));
    return 0;
  }
  if (kind == HOST) {
    if (hredcap < n) {
      if (hred) (void)hipHostFree(hred);
      FL_HIP(hipHostMalloc((void **)&hred, sizeof(double) * (size_t)std::max(n, 64)));
      hredcap = std::max(n, 64);
    }
    FL_HIP(hipMemcpyAsync(hred, dev, sizeof(double) * n, hipMemcpyDeviceToHost, st));
    FL_HIP(hipStreamSynchronize(st));
    if (allred(ctx, hred, n) != 0) return FL_ERR_LIB;
    FL_HIP(hipMemcpyAsync(dev, hred, sizeof(double) * n, hipMemcpyHostToDevice, st));
    return 0;
  }
  return FL_ERR_ARG_WRONGSTATE;
}


void Comm::destroy_oneshot()
{
  if (!owns) {  // a multigrid level: the mailboxes belong to the fine handle
    box = nullptr;
    peers_dev = nullptr;
    oneshot_ready = false;
    return;
  }
  for (void *p : ipc_opened) (void)hipIpcCloseMemHandle(p);
  ipc_opened.clear();
  if (peers_dev) (void)hipFree(peers_dev);
  if (box) (void)hipFree(box);
  peers_dev = nullptr;
  box = nullptr;
  oneshot_ready = false;
  oneshot_calls = 0;
}
void Comm::destroy()
{
  destroy_oneshot();
  if (kind == RCCL && nccl && owns) g_rccl.CommDestroy(nccl);
  for (double *p : hsend)
    if (p) (void)hipHostFree(p);
  for (double *p : hrecv)
    if (p) (void)hipHostFree(p);
  if (hred) (void)hipHostFree(hred);
  hsend.clear();
  hrecv.clear();
  hcap.clear();
  hred = nullptr;
  hredcap = 0;
  nccl = nullptr;
  kind = NONE;
  owns = true;
}

}  // namespace fl

// ------------------------------------------------------------------------------------------------ comm init

extern "C" int fl_comm_unique_id(void *out128)
{
  if (!out128) return FL_ERR_ARG_NULL;
  FL_CHK(g_rccl.load());
  ncclUniqueId id;
  static_assert(sizeof(ncclUniqueId) == FL_UNIQUE_ID_BYTES, "ncclUniqueId size");
  FL_NCCL(g_rccl.GetUniqueId(&id));
  std::memcpy(out128, &id, sizeof(id));
  return FL_SUCCESS;
}

extern "C" int fl_poisson_comm_init_rccl(fl_poisson *h, const void *id128, int rank, int nranks)
{
  if (h) fl_mg_destroy(h);  // the levels of a multigrid hierarchy borrow this handle's communicator: rebuilt on the next solve

  if (!h || !id128) return FL_ERR_ARG_NULL;
  if (nranks != h->dec.ranks[0] * h->dec.ranks[1] * h->dec.ranks[2] || rank < 0 || rank >= nranks) return FL_ERR_ARG_WRONG;
  FL_CHK(g_rccl.load());
  FL_HIP(hipSetDevice(h->device));
  ncclUniqueId id;
  std::memcpy(&id, id128, sizeof(id));
  h->comm.destroy();
  FL_NCCL(g_rccl.CommInitRank(&h->comm.nccl, nranks, id, rank));
  h->comm.kind   = Comm::RCCL;
  h->cheb2_agreed[0] = h->cheb2_agreed[1] = -1;  // a new communicator: the ranks vote again (fl_cheb2_agree)
  h->comm.rank   = rank;
  h->comm.nranks = nranks;
  return FL_SUCCESS;
}

extern "C" int fl_poisson_comm_init_host(fl_poisson *h, fl_exchange_fn xchg, fl_allreduce_fn allred, void *ctx, int rank, int nranks)
{
  if (h) fl_mg_destroy(h);  // the levels of a multigrid hierarchy borrow this handle's communicator: rebuilt on the next solve

  if (!h || !xchg || !allred) return FL_ERR_ARG_NULL;
  if (nranks != h->dec.ranks[0] * h->dec.ranks[1] * h->dec.ranks[2] || rank < 0 || rank >= nranks) return FL_ERR_ARG_WRONG;
  h->comm.destroy();
  h->comm.kind   = Comm::HOST;
  h->cheb2_agreed[0] = h->cheb2_agreed[1] = -1;  // a new communicator: the ranks vote again (fl_cheb2_agree)
  h->comm.xchg   = xchg;
  h->comm.allred = allred;
  h->comm.ctx    = ctx;
  h->comm.rank   = rank;
  h->comm.nranks = nranks;
  return FL_SUCCESS;
}

// ------------------------------------------------------------------------------------------------ one-shot all-reduce (fl_handle.h: OneShotBox)
namespace fl {
// One wave.  Lane l < nranks delivers to peer l and later fetches rank l's slot; every store that a peer waits for is a system-scope release, every
// load of a flag a system-scope acquire (the mailboxes are fine-grained memory, possibly of another device).  A wait gives up after about two
// seconds of wall clock and raises the mailbox's error flag -- a kernel that spins for ever would take the GPU (and its neighbours) down with it.
__global__ void __launch_bounds__(64) k_oneshot_allreduce(OneShotBox *const *boxes, int rank, int nranks, unsigned long long number, double *vals, int n)
{
  const int lane = threadIdx.x, par = (int)(number & 1ull);
  __shared__ double got[NSLOT][NSLOT];
  if (lane < nranks) {
    OneShotBox *peer = boxes[lane];
    for (int a = 0; a < n; ++a) __hip_atomic_store(&peer->slot[par][rank][a], vals[a], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(&peer->seq[par][rank], number, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    OneShotBox     *mine = boxes[rank];
    const long long t0 = wall_clock64();  // 100 MHz
    bool            ok = mine->error == 0;  // sticky: after one timed-out wait every later call gives up at once (NaN sums end the solve)
    while (ok && __hip_atomic_load(&mine->seq[par][lane], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM) != number) {
      if (wall_clock64() - t0 > 200000000ll) {
        ok = false;
        break;
      }
      __builtin_amdgcn_s_sleep(2);
    }
    if (!ok) mine->error = 1;
    for (int a = 0; a < n; ++a) got[lane][a] = ok ? __hip_atomic_load(&mine->slot[par][lane][a], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) : nan("");
  }
  __syncthreads();
  if (lane < n) {
    double sum = 0.;
    for (int r = 0; r < nranks; ++r) sum += got[r][lane];  // rank order: the same bits on every rank
    vals[lane] = sum;
  }
}
void launch_oneshot_allreduce(hipStream_t st, OneShotBox *const *boxes, int rank, int nranks, unsigned long long number, double *vals, int n)
{
  hipLaunchKernelGGL(k_oneshot_allreduce, dim3(1), dim3(64), 0, st, boxes, rank, nranks, number, vals, n);
}
}  // namespace fl

// This rank's mailbox (created by the first call) as a 64-byte hipIpcMemHandle_t for the other PROCESSES, and its address for other handles of
// this process.  The host gathers the handles of all ranks (torch.distributed, MPI, ...) and hands every rank the whole list.
extern "C" int fl_poisson_comm_oneshot_handle(fl_poisson *h, void *ipc_handle64, void **address)
{
  if (!h) return FL_ERR_ARG_NULL;
  if (h->comm.kind == Comm::NONE) return FL_ERR_ARG_WRONGSTATE;
  if (h->comm.nranks > NSLOT) return FL_ERR_SUP;
  FL_HIP(hipSetDevice(h->device));
  if (!h->comm.box) {
    FL_HIP(hipExtMallocWithFlags((void **)&h->comm.box, sizeof(OneShotBox), hipDeviceMallocFinegrained));
    FL_HIP(hipMemset(h->comm.box, 0, sizeof(OneShotBox)));
  }
  if (ipc_handle64) {
    static_assert(sizeof(hipIpcMemHandle_t) == FL_IPC_HANDLE_BYTES, "hipIpcMemHandle_t size");
    hipIpcMemHandle_t hd;
    FL_HIP(hipIpcGetMemHandle(&hd, h->comm.box));
    std::memcpy(ipc_handle64, &hd, sizeof(hd));
  }
  if (address) *address = h->comm.box;
  return FL_SUCCESS;
}
// handles: nranks x 64 bytes in rank order (NULL entries are not allowed), or -- same process -- addresses: nranks mailbox addresses as
// fl_poisson_comm_oneshot_handle returned them.  Exactly one of the two is given.  From then on "allreduce" = 1 routes this handle's scalar
// reductions through the mailboxes (the multigrid levels keep the communicator's own all-reduce).
extern "C" int fl_poisson_comm_oneshot_attach(fl_poisson *h, const void *handles, void *const *addresses)
{
  if (!h || (!handles == !addresses)) return FL_ERR_ARG_NULL;
  Comm &c = h->comm;
  if (c.kind == Comm::NONE || !c.box) return FL_ERR_ARG_WRONGSTATE;
  FL_HIP(hipSetDevice(h->device));
  std::vector<OneShotBox *> peers((size_t)c.nranks, nullptr);
  for (int r = 0; r < c.nranks; ++r) {
    if (r == c.rank) peers[(size_t)r] = c.box;
    else if (addresses) peers[(size_t)r] = (OneShotBox *)addresses[r];
    else {
      hipIpcMemHandle_t hd;
      std::memcpy(&hd, (const char *)handles + (size_t)r * FL_IPC_HANDLE_BYTES, sizeof(hd));
      void *p = nullptr;
      FL_HIP(hipIpcOpenMemHandle(&p, hd, hipIpcMemLazyEnablePeerAccess));
      c.ipc_opened.push_back(p);
      peers[(size_t)r] = (OneShotBox *)p;
    }
    if (!peers[(size_t)r]) return FL_ERR_ARG_NULL;
  }
  if (!c.peers_dev) FL_HIP(hipMalloc((void **)&c.peers_dev, sizeof(OneShotBox *) * NSLOT));
  FL_HIP(hipMemcpy(c.peers_dev, peers.data(), sizeof(OneShotBox *) * peers.size(), hipMemcpyHostToDevice));
  c.oneshot_calls = 0;
  c.oneshot_ready = true;
  return FL_SUCCESS;
}
// 1 if a wait of a one-shot all-reduce on this handle ever ran into its time limit (the sums of that call are NaN)
extern "C" int fl_poisson_comm_oneshot_error(fl_poisson *h, int *error)
{
  if (!h || !error) return FL_ERR_ARG_NULL;
  *error = 0;
  if (!h->comm.box) return FL_SUCCESS;
  FL_HIP(hipSetDevice(h->device));
  OneShotBox host;
  FL_HIP(hipStreamSynchronize(h->stream));
  FL_HIP(hipMemcpy(&host, h->comm.box, sizeof(host), hipMemcpyDeviceToHost));
  *error = host.error;
  return FL_SUCCESS;
}

extern "C" int fl_poisson_comm_info(fl_poisson *h, fl_comm_info *out)
{
  if (!h || !out) return FL_ERR_ARG_NULL;
  std::memset(out, 0, sizeof(*out));
  out->transport = h->comm.kind == Comm::RCCL ? 1 : h->comm.kind == Comm::HOST ? 2 : 0;
  out->rank      = h->comm.rank;
  out->nranks    = h->comm.nranks;
  out->loopback  = h->loopback ? 1 : 0;
  if (h->comm.kind == Comm::RCCL && h->comm.nccl) {  // what the communicator itself says, not what init was told
    FL_NCCL(g_rccl.CommCount(h->comm.nccl, &out->nranks));
    FL_NCCL(g_rccl.CommUserRank(h->comm.nccl, &out->rank));
  }
  if (h->multi) {
    fl_halo_msg plan[12];
    const int   np = fl_halo_messages(h, false, plan);  // between ranks: the loopback self-messages are not counted
    std::vector<int> peers;
    for (int a = 0; a < np; ++a) {
      if (plan[a].send_boundary >= 0) out->halo_bytes += (int64_t)sizeof(double) * (int64_t)fl_plane_size(h, plan[a].send_boundary / 2);
      if (std::find(peers.begin(), peers.end(), plan[a].peer) == peers.end()) peers.push_back(plan[a].peer);
    }
    out->messages   = np;
    out->neighbours = (int)peers.size();
  }
  return FL_SUCCESS;
}

// ------------------------------------------------------------------------------------------------ reductions over the ranks

// All ranks of the handle's communicator have reached this call (and the handle's stream is idle) when it returns: a
// one-double sum over the ranks.  The host mirror sequences file output of the ranks with it (MPI_Barrier in the reference).
extern "C" int fl_poisson_barrier(fl_poisson *h)
{
  if (!h) return FL_ERR_ARG_NULL;
  FL_HIP(hipSetDevice(h->device));
  if (h->multi) {
    FL_HIP(hipMemsetAsync(h->sums, 0, sizeof(double) * NSLOT, h->stream));
    FL_CHK(h->comm.allreduce(h->stream, h->sums, NSLOT));
  }
  FL_HIP(hipStreamSynchronize(h->stream));
  return FL_SUCCESS;
}

// NSLOT host numbers summed over the ranks of the handle's communicator, through h->sums.  A host wait.
static int allreduce_host(fl_poisson *h, double host[NSLOT])
{
  FL_HIP(hipMemcpyAsync(h->sums, host, sizeof(double) * NSLOT, hipMemcpyHostToDevice, h->stream));
  FL_CHK(h->comm.allreduce(h->stream, h->sums, NSLOT));
  FL_HIP(hipMemcpyAsync(host, h->sums, sizeof(double) * NSLOT, hipMemcpyDeviceToHost, h->stream));
  FL_HIP(hipStreamSynchronize(h->stream));
  return 0;
}

// max of one host number over the ranks of the handle's communicator, through the sum all-reduce it has: every rank writes its value into its
// own slot of a zeroed array (at most NSLOT ranks).  A host wait; for set-up quantities only (bounds, estimates).
int fl_allreduce_max(fl_poisson *h, double *v)
{
  if (!h->multi) return 0;
  const int nr = h->comm.nranks;
  if (nr > NSLOT) return FL_ERR_SUP;
  double host[NSLOT] = {0., 0., 0., 0., 0., 0., 0., 0.};
  host[h->comm.rank] = *v;
  FL_CHK(allreduce_host(h, host));
  double mx = host[0];
  for (int a = 1; a < nr; ++a) mx = std::max(mx, host[a]);
  *v = mx;
  return 0;
}

int fl_allreduce_sum(fl_poisson *h, double *v)
{
  if (!h->multi) return 0;
  double host[NSLOT] = {*v, 0., 0., 0., 0., 0., 0., 0.};
  FL_CHK(allreduce_host(h, host));
  *v = host[0];
  return 0;
}

extern "C" int fl_poisson_allreduce_sum(fl_poisson *h, double *host_vals, int n)
{
  if (!h || !host_vals) return FL_ERR_ARG_NULL;
  if (n < 0 || n > NSLOT) return FL_ERR_ARG_OUTOFRANGE;
  if (!h->multi || n == 0) return FL_SUCCESS;
  FL_HIP(hipSetDevice(h->device));
  double host[NSLOT] = {0., 0., 0., 0., 0., 0., 0., 0.};
  std::memcpy(host, host_vals, sizeof(double) * (size_t)n);
  FL_CHK(allreduce_host(h, host));
  std::memcpy(host_vals, host, sizeof(double) * (size_t)n);
  return FL_SUCCESS;
}
