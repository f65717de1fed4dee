// fl_place.hip -- where the padded solver vectors of a handle live: the physical-placement search (one arena, a probed window, side pools)
// and the workspace helpers that hand vectors out (fl_ensure_vec and its kin).
#include <new>

#include "fl_handle.h"

// ------------------------------------------------------------------------------------------------ placement
// Kernels that stream five or six gigabyte-sized vectors in lock step (k_cg_A: reads r, p, x, writes p', q, x) run in one
// of two modes on MI355X, 1.10 ms or 1.27 ms per launch at 512^3.  Measured cause (profiles/r02_placement.md): the mode is
// a property of WHERE IN PHYSICAL MEMORY the vectors live relative to each other.  Vectors that sit in one physically
// contiguous block of HBM -- what back-to-back hipMallocs, and any layout inside the first 16 GiB of one large allocation,
// produce -- are slow at every spacing and alignment; as soon as two or three of the five come from a different block the
// kernel runs 13 % faster (a sliding window of five packed vectors inside one 96 GiB allocation is slow everywhere except
// where it straddles the seams between the driver's blocks, at 16 GiB and 64 GiB into the allocation).
// So placement is no lottery: ONE arena large enough to contain a seam is allocated, a window of five packed vectors slides
// through it (k_cg_A itself is the probe, ~20 positions of a few ms), and the solver vectors are carved out where the window
// was fastest; the vectors outside the window come alternately from the arena's two sides.  Done once per handle, by the
// first fl_ensure_vec of a large handle (tuning knob "placement", default 1) or explicitly by fl_poisson_tune_placement.

// An arena whose physical memory is a row of separately created chunks mapped into one reserved address range (HIP virtual memory
// management).  The search below slides its window through it like through a plain allocation; afterwards the chunks the chosen window
// does not touch are unmapped and released, so the handle keeps the window's own physical memory -- the place the probe measured --
// and nothing else.
struct VmmArena {
  char                                      *va = nullptr;
  size_t                                     size = 0, chunk = 0;
  std::vector<hipMemGenericAllocationHandle_t> handles;
  std::vector<char>                          live;
  size_t bytes_live() const
  {
    size_t n = 0;
    for (char c : live) n += c ? chunk : 0;
    return n;
  }
  void release_outside(size_t lo, size_t hi)  // keeps every chunk that overlaps [lo, hi)
  {
    for (size_t c = 0; c < handles.size(); ++c) {
      const size_t b = c * chunk, e = b + chunk;
      if (live[c] && (e <= lo || b >= hi)) {
        (void)hipMemUnmap(va + b, chunk);
        (void)hipMemRelease(handles[c]);
        live[c] = 0;
      }
    }
  }
  ~VmmArena()
  {
    if (!va) return;
    release_outside(0, 0);
    (void)hipMemAddressFree(va, size);
  }
};
static VmmArena *vmm_arena_create(int device, size_t want, size_t chunk_hint)
{
  hipMemAllocationProp prop = {};
  prop.type                 = hipMemAllocationTypePinned;
  prop.location.type        = hipMemLocationTypeDevice;
  prop.location.id          = device;
  size_t gran = 0;
  if (hipMemGetAllocationGranularity(&gran, &prop, hipMemAllocationGranularityRecommended) != hipSuccess || gran == 0) {
    (void)hipGetLastError();
    return nullptr;
  }
  VmmArena *A = new (std::nothrow) VmmArena;
  if (!A) return nullptr;
  A->chunk = ((chunk_hint + gran - 1) / gran) * gran;
  const size_t n = (want + A->chunk - 1) / A->chunk;
  A->size = n * A->chunk;
  void *va = nullptr;
  if (hipMemAddressReserve(&va, A->size, 0, nullptr, 0) != hipSuccess) {
    (void)hipGetLastError();
    delete A;
    return nullptr;
  }
  A->va = (char *)va;
  hipMemAccessDesc acc = {};
  acc.location         = prop.location;
  acc.flags            = hipMemAccessFlagsProtReadWrite;
  size_t accessible = 0;
  for (size_t c = 0; c < n; ++c) {
    hipMemGenericAllocationHandle_t hd;
    if (hipMemCreate(&hd, A->chunk, &prop, 0) != hipSuccess) break;
    if (hipMemMap(A->va + c * A->chunk, A->chunk, 0, hd, 0) != hipSuccess) {
      (void)hipMemRelease(hd);
      break;
    }
    A->handles.push_back(hd);
    A->live.push_back(1);
    if (hipMemSetAccess(A->va + c * A->chunk, A->chunk, &acc, 1) != hipSuccess) break;
    ++accessible;
  }
  if (accessible != n) {  // a chunk that could not be created, mapped or made accessible: the arena's destructor unmaps and releases what exists
    (void)hipGetLastError();
    delete A;
    return nullptr;
  }
  return A;
}
void fl_vmm_destroy(fl_poisson *h)
{
  if (h->vmm) delete h->vmm;
  h->vmm = nullptr;
}

namespace {
constexpr size_t PL_MIN_VEC   = (size_t)256 << 20;  // smaller vectors: nothing to gain, plain allocations
constexpr size_t PL_SEAM      = (size_t)16 << 30;   // where the first seam of a fresh allocation has been found on every box
constexpr int    PL_WIN       = 5;                   // r, P0, P1, q, xp
constexpr int    PL_SIDE      = 3;                   // pool slots on either side of the window

int place_vectors(fl_poisson *h)
{
  if (h->placed) return 0;
  h->placed = true;  // whatever happens below is final for this handle
  hipStream_t  s    = h->stream;
  const size_t vecb = ((sizeof(double) * h->padlen + ((size_t)2 << 20) - 1) / ((size_t)2 << 20)) * ((size_t)2 << 20);
  const int    nslot = PL_WIN + 2 * PL_SIDE;
  if (vecb < PL_MIN_VEC) return 0;  // small vectors: the kernels are not bandwidth-bound enough to notice; plain allocations
  PlanA plan = plan_cg_A(h->g, 0, 0);
  plan.probe = 1;  // launches k_cg_A_probe / k_cg_Bq_probe: identical code, separate names in profiles
  FL_CHK(fl_ensure_partials(h, plan.nblocks));
  struct Held {  // two scalar blocks (direction buffer parity 0 and 1) and the arenas: whatever is not handed to the handle is released
    KspScal                *p = nullptr;
    std::vector<void *>     arenas;
    std::vector<VmmArena *> vmm;  // parallel to arenas: non-null where the arena is chunk-mapped virtual memory
    ~Held()
    {
      if (p) (void)hipFree(p);
      for (size_t a = 0; a < arenas.size(); ++a) {
        if (vmm[a]) delete vmm[a];
        else if (arenas[a]) (void)hipFree(arenas[a]);
      }
    }
  } sc;
  FL_HIP(hipMalloc((void **)&sc.p, 2 * sizeof(KspScal)));
  {
    KspScal S2[2];
    std::memset(S2, 0, sizeof(S2));
    for (int a = 0; a < 2; ++a) {
      S2[a].beta = 0.5; S2[a].alpha = 1e-3; S2[a].zshift = 1e-4; S2[a].ncell_global = (double)h->ncell; S2[a].maxit = 1 << 30; S2[a].cur = a;
      for (double &al : S2[a].aring) al = 1e-3;
    }
    FL_HIP(hipMemcpy(sc.p, S2, sizeof(S2), hipMemcpyHostToDevice));
  }
  const int verbose = knob(K_placement_verbose);
  // probe = the pair the solver runs: k_cg_A (r, p -> p') and the x-flushing k_cg_Bq of a two-slot ring (p', p_old, r, x -> r, x: every
  // window vector but q).  The further slots of a deeper ring (cg_xdepth > 2) are not in the window: plain allocations.
  auto probe = [&](void *arena, size_t b, double *ms_out) -> int {
    auto          vec = [&](int k) { return (double *)((char *)arena + b + (size_t)k * vecb); };
    const DirRing P   = dir_ring2(vec(1), vec(2));
    auto run = [&](int reps) {
      for (int r = 0; r < reps; ++r)
        for (int par = 0; par < 2; ++par) {
          launch_cg_A(s, h->g, true, plan, vec(0), P, vec(3), vec(4), sc.p + par, h->partial, nullptr, nullptr, 0);
          launch_cg_Bq(s, h->g, true, plan, 2, false, P, vec(0), vec(4), sc.p + par, h->partial, h->partial_stride, nullptr, nullptr, 0);
        }
    };
    // one untimed pair (TLB / L2 warm-up of the new position), then one timed repetition = two pairs (both direction-buffer parities)
    launch_cg_A(s, h->g, true, plan, vec(0), P, vec(3), vec(4), sc.p, h->partial, nullptr, nullptr, 0);
    launch_cg_Bq(s, h->g, true, plan, 2, false, P, vec(0), vec(4), sc.p, h->partial, h->partial_stride, nullptr, nullptr, 0);
    FL_HIP(hipEventRecord(h->ev0, s));
    run(1);
    FL_HIP(hipEventRecord(h->ev1, s));
    FL_HIP(hipStreamSynchronize(s));
    float ms = 0.f;
    FL_HIP(hipEventElapsedTime(&ms, h->ev0, h->ev1));
    *ms_out = ms / 2.;
    return 0;
  };
  // Where the seams of an allocation lie depends on what the device's memory manager handed out before (on most fresh boxes one is
  // found 16 GiB in; on some the whole arena answers flat).  A flat arena is kept allocated -- so that the next one comes from other
  // physical memory -- and the search repeated, at most PL_ARENAS times; the losers are freed at the end.
  constexpr int PL_ARENAS = 3;
  const int use_vmm = knob(K_placement_vmm);  // 1 (default): chunk-mapped arenas, everything but the chosen window is released
  void  *arena = nullptr;
  size_t want = 0, best = 0;
  double first_ms = 0., best_ms = 0.;
  for (int attempt = 0; attempt < PL_ARENAS; ++attempt) {
    size_t freeb = 0, total = 0;
    if (hipMemGetInfo(&freeb, &total) != hipSuccess) break;
    size_t w = ((PL_SEAM + (size_t)(PL_WIN + PL_SIDE) * vecb + ((size_t)1 << 30) - 1) >> 30) << 30;
    const size_t reserve = (size_t)16 << 30;
    if (freeb < w + reserve) {
      if (attempt > 0) break;  // further arenas only while memory is plentiful
      w = freeb > reserve + (size_t)nslot * vecb ? ((freeb - reserve) >> 30) << 30 : 0;
    }
    if (w < (size_t)nslot * vecb) break;  // not enough memory for an arena
    void     *a  = nullptr;
    VmmArena *va = use_vmm ? vmm_arena_create(h->device, w, (size_t)256 << 20) : nullptr;
    if (va) a = va->va;
    else if (hipMalloc(&a, w) != hipSuccess) {
      (void)hipGetLastError();
      break;
    }
    sc.arenas.push_back(a);
    sc.vmm.push_back(va);
    FL_HIP(hipMemsetAsync(a, 0, w, s));
    const size_t lo = (size_t)PL_SIDE * vecb, hi = w - (size_t)(PL_WIN + PL_SIDE) * vecb;
    // coarse pass in steps of one vector (the fast stretch before a seam is four vectors long), then the two half steps next to the best
    const size_t step = std::max(vecb, (((hi - lo) / 32) >> 21) << 21);
    size_t       abest = lo;
    double       afirst = 0., abest_ms = 0.;
    int          nprobe = 0;
    auto         try_at = [&](size_t b) -> int {
      double ms = 0.;
      FL_CHK(probe(a, b, &ms));
      if (verbose) std::fprintf(stderr, "[fluca placement] arena %d, window at %.2f GiB: %.4f ms\n", attempt, (double)b / (double)((size_t)1 << 30), ms);
      if (nprobe++ == 0) afirst = abest_ms = ms;
      if (ms < abest_ms) {
        abest_ms = ms;
        abest    = b;
      }
      return 0;
    };
    for (size_t b = lo; b <= hi; b += step) FL_CHK(try_at(b));
    if (abest_ms <= 0.985 * afirst) {
      const size_t c = abest, half = ((step / 2) >> 21) << 21;
      if (c >= lo + half) FL_CHK(try_at(c - half));
      if (c + half <= hi) FL_CHK(try_at(c + half));
    }
    if (attempt == 0) first_ms = afirst;
    if (!arena || abest_ms < best_ms) {
      arena   = a;
      want    = w;
      best    = abest;
      best_ms = abest_ms;
    }
    if (best_ms <= 0.97 * first_ms) break;  // a seam was found
  }
  if (!arena) return 0;  // no memory for an arena: plain allocations
  // A chunk-mapped arena gives back everything but the chunks under the chosen window: the handle keeps five vectors (plus at most two
  // chunks of 256 MiB of slack), on the very physical memory the probe measured.  (Round 2 kept the whole arena, 16 GiB + 8 vectors;
  // giving it back and allocating "the same place" again -- a filler of the window's offset, then the window -- was tried and does not
  // land on the same physical memory: probe 1.729 ms where the search had found 1.636, profiles/r03_placement.txt.)
  {
    VmmArena *chosen = nullptr;
    for (size_t a = 0; a < sc.arenas.size(); ++a)
      if (sc.arenas[a] == arena) chosen = sc.vmm[a];
    if (chosen) {
      const size_t winb = (size_t)PL_WIN * vecb;
      for (size_t a = 0; a < sc.arenas.size(); ++a)
        if (sc.vmm[a] == chosen) {
          sc.vmm[a]    = nullptr;
          sc.arenas[a] = nullptr;
        }
      // `chosen` left the search's guard above: until the handle owns it, every early return below must give it back
      struct Owner {
        VmmArena *a;
        ~Owner() { delete a; }
      } own{chosen};
      chosen->release_outside(best, best + winb);
      FL_HIP(hipMemsetAsync((char *)arena + best, 0, winb, s));
      double again = 0.;
      const int prc = probe(arena, best, &again);
      if (prc != 0) return prc;
      if (verbose) std::fprintf(stderr, "[fluca placement] window at %.2f GiB kept (%.2f GiB live of %.2f), probe again %.4f ms (search %.4f, first %.4f)\n", (double)best / (double)((size_t)1 << 30), (double)chosen->bytes_live() / (double)((size_t)1 << 30), (double)chosen->size / (double)((size_t)1 << 30), again, best_ms, first_ms);
      FL_HIP(hipMemsetAsync((char *)arena + best, 0, winb, s));
      FL_HIP(hipStreamSynchronize(s));
      own.a          = nullptr;
      h->vmm         = chosen;
      h->arena       = nullptr;  // no side pools: every other vector is a plain allocation
      h->arena_bytes = chosen->bytes_live();
      h->vec_bytes += chosen->bytes_live();
      double **wv[PL_WIN] = {&h->r, &h->P0, &h->P1, &h->q, &h->xp};
      for (int k = 0; k < PL_WIN; ++k) *wv[k] = (double *)((char *)arena + best + (size_t)k * vecb);
      h->nvec += PL_WIN;
      h->placed_ms[0] = first_ms;
      h->placed_ms[1] = again;
      h->placed_at    = (double)best / (double)((size_t)1 << 30);
      return 0;
    }
  }
  for (void *&a : sc.arenas)
    if (a == arena) a = nullptr;  // this one goes to the handle
  // the probes wrote into the arena: ghost layers of fresh solver vectors are zero by contract
  FL_HIP(hipMemsetAsync(arena, 0, want, s));
  FL_HIP(hipStreamSynchronize(s));
  h->arena       = arena;
  h->arena_bytes = want;
  h->vec_bases.push_back(arena);
  h->vec_bytes += want;
  double **win[PL_WIN] = {&h->r, &h->P0, &h->P1, &h->q, &h->xp};
  for (int k = 0; k < PL_WIN; ++k) *win[k] = (double *)((char *)arena + best + (size_t)k * vecb);
  h->pool_next[0] = (char *)arena + best - (size_t)PL_SIDE * vecb;
  h->pool_end[0]  = (char *)arena + best;
  h->pool_next[1] = (char *)arena + best + (size_t)PL_WIN * vecb;
  h->pool_end[1]  = h->pool_next[1] + (size_t)PL_SIDE * vecb;
  h->pool_vec     = vecb;
  h->nvec += PL_WIN;
  h->placed_ms[0] = first_ms;
  h->placed_ms[1] = best_ms;
  h->placed_at    = (double)best / (double)((size_t)1 << 30);
  return 0;
}
}  // namespace

// a padded vector from the arena's side pools (alternating sides), or nullptr when there is no arena / no slot left
static double *pool_take(fl_poisson *h)
{
  if (!h->arena) return nullptr;
  for (int t = 0; t < 2; ++t) {
    const int side = (h->pool_flip + t) & 1;
    if (h->pool_next[side] + h->pool_vec <= h->pool_end[side]) {
      double *v = (double *)h->pool_next[side];
      h->pool_next[side] += h->pool_vec;
      h->pool_flip = side ^ 1;
      return v;
    }
  }
  return nullptr;
}

// Explicit form of the placement step (idempotent; max_tries is kept for source compatibility and only has to be >= 1).
// probe_ms_out: {k_cg_A probe time with the window at the start of the arena (all vectors in one physical block: what plain
// back-to-back allocations give), probe time at the chosen position}; {0, 0} when the handle is too small to be placed.
extern "C" int fl_poisson_tune_placement(fl_poisson *h, int max_tries, double probe_ms_out[2])
{
  if (!h) return FL_ERR_ARG_NULL;
  if (max_tries < 1) return FL_ERR_ARG_OUTOFRANGE;
  FL_HIP(hipSetDevice(h->device));
  if (!h->placed) {
    FL_HIP(hipStreamSynchronize(h->stream));
    // vectors that exist already (a solve ran before this call) are dropped: every solve re-creates what it needs
    fl_mg_destroy(h);
    for (void *p : h->vec_bases) (void)hipFree(p);
    fl_vmm_destroy(h);
    h->vec_bases.clear();
    h->vec_bytes = 0;
    h->nvec = 0;
    for (double **v : {&h->r, &h->P0, &h->P1, &h->q, &h->xp, &h->w0, &h->w1, &h->w2, &h->cd1, &h->rb}) *v = nullptr;
    for (double *&v : h->Pr) v = nullptr;
    FL_CHK(place_vectors(h));
  }
  if (probe_ms_out) {
    probe_ms_out[0] = h->placed_ms[0];
    probe_ms_out[1] = h->placed_ms[1];
  }
  return FL_SUCCESS;
}

// bytes of device memory the handle holds for its padded solver vectors (placement window or arena included)
extern "C" int fl_poisson_vector_bytes(fl_poisson *h, int64_t *bytes_out)
{
  if (!h || !bytes_out) return FL_ERR_ARG_NULL;
  *bytes_out = (int64_t)h->vec_bytes;
  return FL_SUCCESS;
}

// ------------------------------------------------------------------------------------------------ workspace / ghosts

// Padded solver vectors: from the placement window or the pool where the handle has one, else one allocation per vector (placement).
int fl_ensure_vec(fl_poisson *h, double **v)
{
  if (*v) return 0;
  if (!h->placed && h->nvec == 0 && knob(K_placement) > 0 && sizeof(double) * h->padlen >= PL_MIN_VEC) {
    // carves r, P0, P1, q, xp out of one allocation (see "placement" above).  A failure in there (memory short, a probe launch refused)
    // is no reason to fail the caller's solve: whatever the search held is released and the vectors become plain allocations.
    if (place_vectors(h) != 0) {
      (void)hipGetLastError();
      for (double **w : {&h->r, &h->P0, &h->P1, &h->q, &h->xp}) *w = nullptr;
    }
    if (*v) return 0;
  }
  if (double *p = pool_take(h)) {
    *v = p;
    h->nvec++;
    return 0;
  }
  const size_t slot = ((sizeof(double) * h->padlen + 127) / 128) * 128;
  void        *base = nullptr;
  FL_CHK(fl_dev_alloc(h, &base, slot, true));
  h->vec_bases.push_back(base);
  h->vec_bytes += slot;
  h->nvec++;
  *v = (double *)base;
  return 0;
}

// zero a padded vector (ghosts included) on the handle's stream
int fl_zero_vec(fl_poisson *h, double *v)
{
  FL_HIP(hipMemsetAsync(v, 0, sizeof(double) * h->padlen, h->stream));
  return 0;
}

int fl_ensure_hist(fl_poisson *h, int nhist)
{
  if (h->hist_cap >= nhist) return 0;
  if (h->hist) {
    FL_HIP(hipStreamSynchronize(h->stream));
    FL_HIP(hipFree(h->hist));
    h->hist = nullptr;
  }
  FL_CHK(fl_dev_alloc(h, (void **)&h->hist, sizeof(double) * nhist, true));
  h->hist_cap = nhist;
  return 0;
}

int fl_ensure_partials(fl_poisson *h, int nblocks)
{
  const int want = std::max(nblocks, (int)MAX_PARTIAL_BLOCKS);
  if (h->partial && h->partial_stride >= want) return 0;
  if (h->partial) {
    FL_HIP(hipStreamSynchronize(h->stream));
    FL_HIP(hipFree(h->partial));
    h->partial = nullptr;
  }
  FL_CHK(fl_dev_alloc(h, (void **)&h->partial, sizeof(double) * (size_t)want * NSLOT, true));
  h->partial_stride = want;
  return 0;
}

