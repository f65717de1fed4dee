// fl_api.hip -- C-ABI entry points of libflucahip.so (see include/fluca_hip.h): the handle and its operator entry points, plain device memory,
// the dispatch of fl_poisson_solve and the fldbg_* hooks.  Knobs: fl_knobs.cpp; vector placement: fl_place.hip; ghost exchanges:
// fl_halo.hip; transports: fl_comm.hip; Krylov drivers: fl_ksp.hip, fl_mg.hip.
#include "fl_handle.h"

int fl_dev_alloc(fl_poisson *h, void **p, size_t bytes, bool zero)
{
  FL_HIP(hipMalloc(p, bytes ? bytes : 8));
  if (zero) FL_HIP(hipMemsetAsync(*p, 0, bytes ? bytes : 8, h->stream));
  return 0;
}

template <class T>
static int upload_table(fl_poisson *h, const std::vector<T> &host, const T **dev, int shift)
{
  void *p = nullptr;
  FL_HIP(hipMalloc(&p, sizeof(T) * std::max<size_t>(host.size(), 1)));
  FL_HIP(hipMemcpy(p, host.data(), sizeof(T) * host.size(), hipMemcpyHostToDevice));
  h->tables.push_back(p);
  *dev = (const T *)p + shift;
  return 0;
}

// "abi N": bumped whenever a struct of include/fluca_hip.h grows or an entry point changes its meaning (FL_ABI_VERSION there): a caller built
// against another header must not be handed this library.  5: fl_ksp_opts carries cg_single_reduction (round 3's trailing field), the
// momentum solve accepts FL_KSP_CHEBYSHEV, fl_momentum_gershgorin / fl_momentum_chebyshev_interval exist.  7: owner-rank IBM markers
// (fl_ibm_owned_select / fl_ibm_create_owned / fl_ibm_owned_counts; fl_ibm_update / _interp / _spread are collective on such a set).  8: owner-rank markers migrate
// (fl_ibm_migrate / fl_ibm_owned_fetch).
extern "C" const char *fl_build_id(void);  // lib/fl_build_id.cpp, written by fluca_amd/build.py: a hash over every source, header and compiler flag
extern "C" const char *fl_version(void)
{
  static const std::string v = std::string("fluca_amd 0.3 (gfx950, abi 8, sources ") + fl_build_id() + ")";
  return v.c_str();
}
extern "C" int fl_abi_version(void) { return FL_ABI_VERSION; }

extern "C" void fl_ksp_opts_default(fl_ksp_opts *o)
{
  if (!o) return;
  std::memset(o, 0, sizeof(*o));
  o->type             = FL_KSP_CG;
  o->pc               = FL_PC_JACOBI;
  o->norm_type        = FL_NORM_PRECONDITIONED;
  o->remove_nullspace = 1;
  o->maxit            = 10000;
  o->rtol             = 1e-5;
  o->atol             = 1e-50;
  o->dtol             = 1e5;
  o->check_every      = 16;
}

// everything that can fail after the handle exists; the caller destroys the handle on any error
static int poisson_init(fl_poisson *h, const fl_grid *grid, const int bc[6], double kappa, const fl_decomp *decomp, int device)
{
  h->device     = device;
  h->kappa      = kappa;
  std::memcpy(h->bc, bc, sizeof(int) * 6);
  for (int d = 0; d < 3; ++d) {
    int rc = build_axis(h->ax[d], grid->n[d], grid->xf[d], grid->xc[d], bc[2 * d], bc[2 * d + 1], kappa);
    if (rc) return rc;
  }
  if (decomp) h->dec = *decomp;
  else
    for (int d = 0; d < 3; ++d) {
      h->dec.ranks[d] = 1;
      h->dec.coord[d] = 0;
      h->dec.lo[d]    = 0;
      h->dec.len[d]   = grid->n[d];
    }
  int periodic[3];
  for (int d = 0; d < 3; ++d) {
    const fl_decomp &D = h->dec;
    periodic[d]        = h->ax[d].periodic;
    if (D.ranks[d] < 1 || D.coord[d] < 0 || D.coord[d] >= D.ranks[d] || D.len[d] < 1 || D.lo[d] < 0 || D.lo[d] + D.len[d] > grid->n[d] || D.len[d] > 100000) {
      return FL_ERR_ARG_OUTOFRANGE;
    }
    if ((D.coord[d] == 0) != (D.lo[d] == 0) || (D.coord[d] == D.ranks[d] - 1) != (D.lo[d] + D.len[d] == grid->n[d])) {
      return FL_ERR_ARG_WRONG;
    }
    h->wrap_local[d] = periodic[d] && D.ranks[d] == 1;
  }
  h->multi = h->dec.ranks[0] * h->dec.ranks[1] * h->dec.ranks[2] > 1;
  {
    if (knob(K_comm_loopback) != 0 && !h->multi && (periodic[0] || periodic[1] || periodic[2])) {
      h->loopback = h->comm.loopback = true;
      h->multi    = true;
      for (int d = 0; d < 3; ++d) h->wrap_local[d] = false;
    }
  }
  for (int b = 0; b < 6; ++b) h->nbr[b] = h->multi ? fl_decomp_neighbor(&h->dec, periodic, b) : -1;

  FL_HIP(hipSetDevice(device));
  FL_HIP(hipStreamCreateWithFlags(&h->own_stream, hipStreamNonBlocking));
  h->stream = h->own_stream;
  FL_HIP(hipEventCreate(&h->ev0));
  FL_HIP(hipEventCreate(&h->ev1));

  // ---- local tables ---------------------------------------------------------------------------------------------
  GridP &g = h->g;
  std::memset(&g, 0, sizeof(g));
  g.nx = (int)h->dec.len[0];
  g.ny = (int)h->dec.len[1];
  g.nz = (int)h->dec.len[2];
  int fl_[3];
  for (int d = 0; d < 3; ++d) {
    const bool last = h->dec.coord[d] == h->dec.ranks[d] - 1;
    fl_[d]          = (int)h->dec.len[d] + ((last && !h->ax[d].periodic) ? 1 : 0);
  }
  g.fx    = fl_[0];
  g.fy    = fl_[1];
  g.fz    = fl_[2];
  // Ghost width of the padded layout: 1 = the reference's star stencil (cart.c:66,91), what every operator needs; 2 where a neighbouring RANK
  // sits behind a boundary, so that the two-deep exchange of fl_fill_ghosts_deep has somewhere to put its second layer and the fused
  // two-step smoother (k_cheb2) can run on several ranks.  Kernels only ever see (off0, sx, sxy): the width is a property of the handle,
  // not of the kernels.  FLUCA_GHOST_WIDTH=2 forces the wide layout on a single rank (tests: the whole suite must not care).
  {
    const int forced = knob(K_ghost_width);
    h->gw            = forced > 0 ? forced : (h->multi && !h->loopback ? 2 : 1);
    if (h->gw < 1 || h->gw > 2) h->gw = 1;
  }
  const int gw = h->gw;
  g.sx    = ((PADX + g.nx + gw + 15) / 16) * 16;
  g.sxy   = (int64_t)g.sx * (g.ny + 2 * gw);
  g.off0  = (int64_t)gw * g.sxy + (int64_t)gw * g.sx + PADX;
  g.kappa = kappa;
  h->padlen = (size_t)g.sxy * (g.nz + 2 * gw) + 256;  // doubles spanned by one vector (interleaved: by the whole slab)
  h->ncell  = (int64_t)g.nx * g.ny * g.nz;
  h->nface[0] = (int64_t)g.fx * g.ny * g.nz;
  h->nface[1] = (int64_t)g.nx * g.fy * g.nz;
  h->nface[2] = (int64_t)g.nx * g.ny * g.fz;
  const double inf = std::numeric_limits<double>::infinity();
  for (int d = 0; d < 3; ++d) {
    const Axis   &A  = h->ax[d];
    const int64_t lo = h->dec.lo[d], len = h->dec.len[d], n = A.n;
    std::vector<double> sl(len + 2), sc(len + 2), sh(len + 2), idx(len);
    for (int64_t i = -1; i <= len; ++i) {
      int64_t gi = lo + i;
      bool    in = true;
      if (gi < 0 || gi >= n) {
        if (A.periodic) gi = (gi + n) % n;
        else in = false;
      }
      sl[i + 1] = in ? A.sl[gi] : 0.;
      sc[i + 1] = in ? A.sc[gi] : inf;  // wall ghost: 1/diag = 0
      sh[i + 1] = in ? A.sh[gi] : 0.;
    }
    for (int64_t i = 0; i < len; ++i) idx[i] = A.idx[lo + i];
    std::vector<double> ga0(fl_[d]), ga1(fl_[d]);
    std::vector<int>    gc0(fl_[d]);
    for (int f = 0; f < fl_[d]; ++f) {
      ga0[f] = A.ga0[lo + f];
      ga1[f] = A.ga1[lo + f];
      gc0[f] = (int)(A.gc0[lo + f] - lo);
    }
    std::vector<int>    Gs(len);
    std::vector<double> Gv0(len), Gv1(len), Gv2(len);
    for (int64_t i = 0; i < len; ++i) {
      Gs[i]  = (int)(A.Gs[lo + i] - lo);
      Gv0[i] = A.Gv0[lo + i];
      Gv1[i] = A.Gv1[lo + i];
      Gv2[i] = A.Gv2[lo + i];
      if (Gs[i] < -1 || Gs[i] + (Gv2[i] != 0. ? 2 : 1) > len) {
        // a one-sided wall row that leaves the block + its single ghost layer
        return FL_ERR_SUP;
      }
    }
    int rc = 0;
    rc |= upload_table(h, sl, &g.sl[d], 1);
    rc |= upload_table(h, sc, &g.sc[d], 1);
    rc |= upload_table(h, sh, &g.sh[d], 1);
    rc |= upload_table(h, idx, &g.idx[d], 0);
    rc |= upload_table(h, ga0, &g.ga0[d], 0);
    rc |= upload_table(h, ga1, &g.ga1[d], 0);
    rc |= upload_table(h, gc0, &g.gc0[d], 0);
    rc |= upload_table(h, Gs, &g.Gs[d], 0);
    rc |= upload_table(h, Gv0, &g.Gv0[d], 0);
    rc |= upload_table(h, Gv1, &g.Gv1[d], 0);
    rc |= upload_table(h, Gv2, &g.Gv2[d], 0);
    if (rc) return FL_ERR_GPU;
  }
  FL_HIP(hipMalloc((void **)&h->scal, sizeof(KspScal)));
  FL_HIP(hipHostMalloc((void **)&h->scal_host, sizeof(KspScal)));
  FL_HIP(hipMalloc((void **)&h->sums, sizeof(double) * NSLOT));
  FL_HIP(hipMalloc((void **)&h->tickets, sizeof(unsigned) * 2));
  FL_HIP(hipMemset(h->tickets, 0, sizeof(unsigned) * 2));
  return FL_SUCCESS;
}

extern "C" int fl_poisson_create(const fl_grid *grid, const int bc[6], double kappa, const fl_decomp *decomp, int device, fl_poisson **out)
{
  if (!grid || !bc || !out) return FL_ERR_ARG_NULL;
  *out = nullptr;
  for (int d = 0; d < 3; ++d)
    if (grid->n[d] < 1 || grid->n[d] > (int64_t)1 << 30 || !grid->xf[d]) return FL_ERR_ARG_OUTOFRANGE;
  if (!(kappa > 0.) || !std::isfinite(kappa)) return FL_ERR_ARG_OUTOFRANGE;
  fl_poisson *h  = new fl_poisson();
  const int   rc = poisson_init(h, grid, bc, kappa, decomp, device);
  if (rc) {
    fl_poisson_destroy(h);  // releases whatever was created before the failure
    return rc;
  }
  *out = h;
  return FL_SUCCESS;
}

extern "C" int fl_poisson_destroy(fl_poisson *h)
{
  if (!h) return FL_SUCCESS;
  (void)hipSetDevice(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  fl_mg_destroy(h);
  h->comm.destroy();
  for (SmoothSeq &q : h->smooth_seq)
    if (q.dev) (void)hipFree(q.dev);
  for (void *p : h->tables) (void)hipFree(p);
  for (void *p : h->vec_bases) (void)hipFree(p);
  fl_vmm_destroy(h);
  for (double *p : {h->partial, h->sums, h->hist})
    if (p) (void)hipFree(p);
  for (int b = 0; b < 6; ++b) {
    if (h->fsend[b]) (void)hipFree(h->fsend[b]);
    if (h->frecv[b]) (void)hipFree(h->frecv[b]);
    if (h->xsend[b]) (void)hipFree(h->xsend[b]);
    if (h->xrecv[b]) (void)hipFree(h->xrecv[b]);
  }
  for (int d = 0; d < 3; ++d) {
    if (h->hiface[d]) (void)hipFree(h->hiface[d]);
    if (h->loface_send[d]) (void)hipFree(h->loface_send[d]);
  }
  if (h->scal) (void)hipFree(h->scal);
  if (h->tickets) (void)hipFree(h->tickets);
  if (h->scal_host) (void)hipHostFree(h->scal_host);
  if (h->comm_stream) (void)hipStreamSynchronize(h->comm_stream);
  if (h->ev_packed) (void)hipEventDestroy(h->ev_packed);
  if (h->ev_ghosts) (void)hipEventDestroy(h->ev_ghosts);
  if (h->ev_upload) (void)hipEventDestroy(h->ev_upload);
  if (h->comm_stream) (void)hipStreamDestroy(h->comm_stream);
  if (h->ev0) (void)hipEventDestroy(h->ev0);
  if (h->ev1) (void)hipEventDestroy(h->ev1);
  if (h->own_stream) (void)hipStreamDestroy(h->own_stream);
  delete h;
  return FL_SUCCESS;
}

extern "C" int fl_poisson_set_stream(fl_poisson *h, void *hip_stream)
{
  if (!h) return FL_ERR_ARG_NULL;
  h->stream = hip_stream ? (hipStream_t)hip_stream : h->own_stream;
  fl_mg_set_stream(h);
  return FL_SUCCESS;
}

extern "C" int fl_poisson_synchronize(fl_poisson *h)
{
  if (!h) return FL_ERR_ARG_NULL;
  FL_HIP(hipStreamSynchronize(h->stream));
  return FL_SUCCESS;
}

extern "C" int fl_poisson_sizes(const fl_poisson *h, int64_t out[4])
{
  if (!h || !out) return FL_ERR_ARG_NULL;
  out[0] = h->ncell;
  out[1] = h->nface[0];
  out[2] = h->nface[1];
  out[3] = h->nface[2];
  return FL_SUCCESS;
}

// ------------------------------------------------------------------------------------------------ operator entry points

extern "C" int fl_poisson_apply(fl_poisson *h, const double *x_dev, double *y_dev)
{
  if (!h || !x_dev || !y_dev) return FL_ERR_ARG_NULL;
  FL_HIP(hipSetDevice(h->device));
  FL_CHK(fl_ensure_vec(h, &h->w0));
  launch_pad_copy(h->stream, h->g, x_dev, h->w0);
  FL_CHK(fl_fill_ghosts(h, h->w0));
  FL_CHK(fl_apply_tiled(h, h->w0, y_dev, 1));
  FL_HIP(hipGetLastError());
  return FL_SUCCESS;
}

extern "C" int fl_poisson_diagonal(fl_poisson *h, double *d_dev)
{
  if (!h || !d_dev) return FL_ERR_ARG_NULL;
  FL_HIP(hipSetDevice(h->device));
  launch_diagonal(h->stream, h->g, d_dev);
  FL_HIP(hipGetLastError());
  return FL_SUCCESS;
}

extern "C" int fl_poisson_rhs(fl_poisson *h, const double *Vx, const double *Vy, const double *Vz, const double *contrhs, double *b)
{
  if (!h || !Vx || !Vy || !Vz || !b) return FL_ERR_ARG_NULL;
  FL_HIP(hipSetDevice(h->device));
  const double *V[3] = {Vx, Vy, Vz};
  FL_CHK(fl_fill_hifaces(h, V));  // the high face of the last owned cell belongs to the next rank (or is the periodic image of face 0)
  launch_rhs(h->stream, h->g, Vx, Vy, Vz, h->hiface[0], h->hiface[1], h->hiface[2], contrhs, b);
  FL_HIP(hipGetLastError());
  return FL_SUCCESS;
}

// The route fl_poisson_project takes for these pointers (host arithmetic; fldbg_project_path reports it).  The last line restates the `pairs`
// rule of launch_project_all, which stays where it is: the text of fl_kernels.hip is tied to the counter passes bench.py quotes
// (fluca_amd/provenance.py).  tests/test_gpu_caller_arrays.py holds both branches to the same bits.
enum { PROJECT_SIX_DIRECT = 0, PROJECT_SIX_PADDED = 1, PROJECT_ALL_PAIRS = 2, PROJECT_ALL_SINGLE = 3 };
static int project_path(const fl_poisson *h, const double *p_dev, double *const v[3], double *const V[3])
{
  // all six arrays (PCApply_ABF's call), one rank: k_project_six reads the caller's p itself -- no padded copy, no ghost layers
  if (!h->multi && project_six_usable(h->g, p_dev, v, V)) return PROJECT_SIX_DIRECT;
  if (project_six_usable(h->g, nullptr, v, V)) return PROJECT_SIX_PADDED;  // several ranks: the same kernel on the padded p
  int pairs = h->g.nx % 2 == 0;  // any subset of the six arrays, one pass over p: 16-byte accesses for even rows and aligned bases
  for (int d = 0; d < 3; ++d)
    if ((v[d] && (reinterpret_cast<uintptr_t>(v[d]) & 15)) || (d > 0 && V[d] && (reinterpret_cast<uintptr_t>(V[d]) & 15))) pairs = 0;
  return pairs ? PROJECT_ALL_PAIRS : PROJECT_ALL_SINGLE;
}

extern "C" int fl_poisson_project(fl_poisson *h, const double *p_dev, double *vx, double *vy, double *vz, double *Vx, double *Vy, double *Vz)
{
  if (!h || !p_dev) return FL_ERR_ARG_NULL;
  FL_HIP(hipSetDevice(h->device));
  double *v[3] = {vx, vy, vz}, *V[3] = {Vx, Vy, Vz};
  const int path = project_path(h, p_dev, v, V);
  if (path == PROJECT_SIX_DIRECT) {
    int per = 0;
    for (int d = 0; d < 3; ++d) per |= h->wrap_local[d] ? (1 << d) : 0;
    launch_project_six(h->stream, h->g, p_dev, true, per, v, V);
    FL_HIP(hipGetLastError());
    return FL_SUCCESS;
  }
  FL_CHK(fl_ensure_vec(h, &h->w0));
  launch_pad_copy(h->stream, h->g, p_dev, h->w0);
  FL_CHK(fl_fill_ghosts(h, h->w0));
  if (path == PROJECT_SIX_PADDED) {
    launch_project_six(h->stream, h->g, h->w0, false, 0, v, V);
    FL_HIP(hipGetLastError());
    return FL_SUCCESS;
  }
  launch_project_all(h->stream, h->g, h->w0, v, V);  // any subset of the six arrays, one pass over p; decides on the pairs itself
  FL_HIP(hipGetLastError());
  return FL_SUCCESS;
}

// Not part of the public C-ABI (tests/test_gpu_caller_arrays.py): which route fl_poisson_project takes for these pointers -- 0 k_project_six on
// the caller's p, 1 k_project_six on the padded p, 2 k_project_all with 16-byte accesses to the caller's arrays, 3 k_project_all with 8-byte
// accesses.  Host arithmetic on the pointers' values only: nothing is read, written or launched.
extern "C" int fldbg_project_path(fl_poisson *h, const double *p_dev, double *vx, double *vy, double *vz, double *Vx, double *Vy, double *Vz, int *path)
{
  if (!h || !p_dev || !path) return FL_ERR_ARG_NULL;
  double *v[3] = {vx, vy, vz}, *V[3] = {Vx, Vy, Vz};
  *path = project_path(h, p_dev, v, V);
  return FL_SUCCESS;
}

extern "C" int fl_poisson_gst_bc(fl_poisson *h, int boundary, const double *pb_dev, double *V_dev)
{
  if (!h || !pb_dev || !V_dev) return FL_ERR_ARG_NULL;
  if (boundary < 0 || boundary > 5) return FL_ERR_ARG_OUTOFRANGE;
  const int d = boundary / 2, side = boundary % 2;
  if (h->bc[boundary] != FL_BC_PRESSURE_OUTLET) return FL_SUCCESS;
  const bool touches = side ? (h->dec.coord[d] == h->dec.ranks[d] - 1) : (h->dec.coord[d] == 0);
  if (!touches) return FL_SUCCESS;
  FL_HIP(hipSetDevice(h->device));
  launch_gst_bc(h->stream, h->g, pb_dev, V_dev, d, side, side ? h->ax[d].bcc_hi : h->ax[d].bcc_lo);
  FL_HIP(hipGetLastError());
  return FL_SUCCESS;
}

// The two shapes every boundary-condition vector of the reference has: a value per boundary face, written into the boundary
// faces of a face array (INSERT) or added to the cells next to the boundary (ADD).
static bool touches_boundary(const fl_poisson *h, int boundary)
{
  const int d = boundary / 2, side = boundary % 2;
  if (h->ax[d].periodic) return false;
  return side ? (h->dec.coord[d] == h->dec.ranks[d] - 1) : (h->dec.coord[d] == 0);
}

extern "C" int fl_boundary_set_faces(fl_poisson *h, int boundary, double coeff, const double *plane_dev, double *face_dev)
{
  if (!h || !plane_dev || !face_dev) return FL_ERR_ARG_NULL;
  if (boundary < 0 || boundary > 5) return FL_ERR_ARG_OUTOFRANGE;
  if (!touches_boundary(h, boundary)) return FL_SUCCESS;
  FL_HIP(hipSetDevice(h->device));
  launch_gst_bc(h->stream, h->g, plane_dev, face_dev, boundary / 2, boundary % 2, coeff);
  FL_HIP(hipGetLastError());
  return FL_SUCCESS;
}

extern "C" int fl_boundary_add_faces(fl_poisson *h, int boundary, double coeff, const double *plane_dev, double *face_dev)
{
  if (!h || !plane_dev || !face_dev) return FL_ERR_ARG_NULL;
  if (boundary < 0 || boundary > 5) return FL_ERR_ARG_OUTOFRANGE;
  if (!touches_boundary(h, boundary)) return FL_SUCCESS;
  FL_HIP(hipSetDevice(h->device));
  launch_gst_bc(h->stream, h->g, plane_dev, face_dev, boundary / 2, boundary % 2, coeff, 1);
  FL_HIP(hipGetLastError());
  return FL_SUCCESS;
}

extern "C" int fl_boundary_add_cells(fl_poisson *h, int boundary, double coeff, const double *plane_dev, double *cell_dev)
{
  if (!h || !plane_dev || !cell_dev) return FL_ERR_ARG_NULL;
  if (boundary < 0 || boundary > 5) return FL_ERR_ARG_OUTOFRANGE;
  if (!touches_boundary(h, boundary)) return FL_SUCCESS;
  FL_HIP(hipSetDevice(h->device));
  launch_bc_add_cells(h->stream, h->g, plane_dev, cell_dev, boundary / 2, boundary % 2, coeff);
  FL_HIP(hipGetLastError());
  return FL_SUCCESS;
}

extern "C" int fl_pressure_update(fl_poisson *h, int first, const double *dp, const double *p0, double *phalf, double *p)
{
  if (!h || !dp || !phalf || !p || (first && !p0)) return FL_ERR_ARG_NULL;
  FL_HIP(hipSetDevice(h->device));
  launch_pressure_update(h->stream, h->ncell, first, dp, p0, phalf, p);
  FL_HIP(hipGetLastError());
  return FL_SUCCESS;
}

extern "C" int fl_poisson_solve(fl_poisson *h, const double *b_dev, double *x_dev, const fl_ksp_opts *opts, fl_ksp_stats *stats)
{
  if (!h || !b_dev || !x_dev || !opts || !stats) return FL_ERR_ARG_NULL;
  if (opts->maxit < 0 || opts->maxit > 10000000) return FL_ERR_ARG_OUTOFRANGE;
  if (opts->pc != FL_PC_NONE && opts->pc != FL_PC_JACOBI && opts->pc != FL_PC_MG) return FL_ERR_SUP;
  if (opts->initial_guess_nonzero) return FL_ERR_SUP;  // the Schur solvers start from zero, as the reference's kspS does (nsbasic.c:250-251)
  FL_HIP(hipSetDevice(h->device));
  std::memset(stats, 0, sizeof(*stats));
  if (opts->pc == FL_PC_MG) {
    if (opts->type != FL_KSP_CG) return FL_ERR_SUP;
    if (opts->cg_single_reduction) return FL_ERR_SUP;  // the cycle's sums ride on its last smoothing sweep: no single-reduction form of that loop is built
    return fl_solve_cg_mg(h, b_dev, x_dev, opts, stats);
  }
  switch (opts->type) {
  case FL_KSP_CG:
    if (opts->norm_type < 0 || opts->norm_type > FL_NORM_NONE) return FL_ERR_ARG_OUTOFRANGE;
    if (opts->cg_single_reduction) return fl_solve_cg_sr(h, b_dev, x_dev, opts, stats);  // -ksp_cg_single_reduction
    return fl_solve_cg(h, b_dev, x_dev, opts, stats);
  case FL_KSP_BCGS:
    // KSPBCGS: left preconditioning, preconditioned residual norm only
    if (opts->norm_type != FL_NORM_PRECONDITIONED) return FL_ERR_SUP;
    return fl_solve_bcgs(h, b_dev, x_dev, opts, stats);
  case FL_KSP_CHEBYSHEV:
    if (opts->norm_type < 0 || opts->norm_type > FL_NORM_NONE) return FL_ERR_ARG_OUTOFRANGE;
    return fl_solve_cheb(h, b_dev, x_dev, opts, stats);
  default:
    return FL_ERR_SUP;
  }
}

extern "C" int fl_poisson_gershgorin(const fl_poisson *h, int pc, double *bound)
{
  if (!h || !bound) return FL_ERR_ARG_NULL;
  if (pc != FL_PC_NONE && pc != FL_PC_JACOBI) return FL_ERR_ARG_OUTOFRANGE;
  *bound = fl_gershgorin_bound(h, pc == FL_PC_JACOBI);
  return FL_SUCCESS;
}

// ------------------------------------------------------------------------------------------------ plain device memory

extern "C" int fl_current_device(int *device)
{
  if (!device) return FL_ERR_ARG_NULL;
  FL_HIP(hipGetDevice(device));
  return FL_SUCCESS;
}

extern "C" int fl_malloc(int device, size_t bytes, void **dev_out)
{
  if (!dev_out) return FL_ERR_ARG_NULL;
  *dev_out = nullptr;
  FL_HIP(hipSetDevice(device));
  if (hipMalloc(dev_out, bytes ? bytes : 8) != hipSuccess) return FL_ERR_MEM;
  // hipMemset on the null stream is asynchronous and the handles work on non-blocking streams, which do not wait for
  // the null stream: finish it here, or the zeroes can land on top of the first results written into this buffer.
  FL_HIP(hipMemset(*dev_out, 0, bytes ? bytes : 8));
  FL_HIP(hipDeviceSynchronize());
  return FL_SUCCESS;
}
extern "C" int fl_free(int device, void *dev)
{
  if (!dev) return FL_SUCCESS;
  FL_HIP(hipSetDevice(device));
  FL_HIP(hipFree(dev));
  return FL_SUCCESS;
}
extern "C" int fl_memcpy_h2d(int device, void *dev, const void *host, size_t bytes)
{
  if (!dev || !host) return FL_ERR_ARG_NULL;
  FL_HIP(hipSetDevice(device));
  FL_HIP(hipDeviceSynchronize());  // whatever still reads or writes `dev` on a handle's stream finishes first
  FL_HIP(hipMemcpy(dev, host, bytes, hipMemcpyHostToDevice));
  FL_HIP(hipDeviceSynchronize());
  return FL_SUCCESS;
}
// Page-locked host memory and a copy out of it that is ordered on the handle's stream like a kernel: no device-wide wait on either side (the C host
// mirror hands over some thirty boundary planes per time step; fl_memcpy_h2d drains the device twice per plane).
extern "C" int fl_malloc_host(size_t bytes, void **host_out)
{
  if (!host_out) return FL_ERR_ARG_NULL;
  *host_out = nullptr;
  if (hipHostMalloc(host_out, bytes ? bytes : 8, hipHostMallocDefault) != hipSuccess) return FL_ERR_MEM;
  return FL_SUCCESS;
}
extern "C" int fl_free_host(void *host)
{
  if (!host) return FL_SUCCESS;
  FL_HIP(hipHostFree(host));
  return FL_SUCCESS;
}
extern "C" int fl_poisson_upload(fl_poisson *h, void *dev, const void *host, size_t bytes)
{
  if (!h || !dev || !host) return FL_ERR_ARG_NULL;
  FL_HIP(hipSetDevice(h->device));
  if (!h->ev_upload) FL_HIP(hipEventCreateWithFlags(&h->ev_upload, hipEventDisableTiming));
  FL_HIP(hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, h->stream));
  FL_HIP(hipEventRecord(h->ev_upload, h->stream));
  return FL_SUCCESS;
}
extern "C" int fl_poisson_upload_fence(fl_poisson *h)
{
  if (!h) return FL_ERR_ARG_NULL;
  if (h->ev_upload) FL_HIP(hipEventSynchronize(h->ev_upload));
  return FL_SUCCESS;
}
extern "C" int fl_memcpy_d2h(int device, void *host, const void *dev, size_t bytes)
{
  if (!dev || !host) return FL_ERR_ARG_NULL;
  FL_HIP(hipSetDevice(device));
  FL_HIP(hipDeviceSynchronize());
  FL_HIP(hipMemcpy(host, dev, bytes, hipMemcpyDeviceToHost));
  return FL_SUCCESS;
}

// ------------------------------------------------------------------------------------------------ kernel micro-bench (bench.py, tools/sbench.py)
// Not part of the public C-ABI (not declared in fluca_hip.h): times one kernel in isolation with HIP events.
//   kernel 0: k_cg_A on 128 x (NW * RY) tiles, ry = 10 * RY + NW, nchunk z chunks (0: the chunking rule), pf / 100 = XCD-contiguous block order
//   kernel 2: streaming reference with ry reads / pf writes   3: parametric stream, ry = 10 * NR + NW, pf = 10 * U + NT, nchunk = blocks
extern "C" int fldbg_bench(fl_poisson *h, int kernel, int ry, int pf, int nchunk, int reps, const double *src_dev, double *ms_out, int *nblocks_out)
{
  if (!h || !ms_out) return FL_ERR_ARG_NULL;
  if (kernel != 0 && kernel != 2 && kernel != 3) return FL_ERR_SUP;
  FL_HIP(hipSetDevice(h->device));
  const GridP &g = h->g;
  for (double **v : {&h->r, &h->P0, &h->P1, &h->q, &h->xp, &h->w0}) FL_CHK(fl_ensure_vec(h, v));
  hipStream_t s = h->stream;
  if (src_dev) {
    launch_pad_copy(s, g, src_dev, h->r);
    launch_pad_copy(s, g, src_dev, h->P0);
    launch_pad_copy(s, g, src_dev, h->xp);
    launch_pad_copy(s, g, src_dev, h->q);
  }
  PlanA plan = kernel == 0 ? plan_tiles(g, ry / 10, ry % 10, nchunk, 512) : plan_cg_A(g, 0, 0);
  if (kernel == 0) plan.remap = pf / 100;
  FL_CHK(fl_ensure_partials(h, plan.nblocks));
  KspScal &S = *h->scal_host;
  std::memset(&S, 0, sizeof(S));
  S.beta = 0.5; S.alpha = 1e-3; S.zshift = 1e-4; S.ncell_global = (double)h->ncell; S.maxit = 1 << 30; S.pending_x = 1; S.nullspace = 1; S.rz = 1.;
  FL_HIP(hipMemcpyAsync(h->scal, h->scal_host, sizeof(KspScal), hipMemcpyHostToDevice, s));
  auto once = [&]() {
    if (kernel == 0) launch_cg_A(s, g, true, plan, h->r, dir_ring2(h->P0, h->P1), h->q, h->xp, h->scal, h->partial, nullptr, nullptr, 0);
    else if (kernel == 2) launch_stream_ref(s, ry, pf, (int64_t)(h->padlen - 256) / 2, h->r, h->P0, h->xp, h->P1, h->q, h->w0);
    else launch_stream_par(s, ry / 10, ry % 10, pf / 10, pf % 10, nchunk, (int64_t)(h->padlen - 256) / 2, h->r, h->P0, h->xp, h->P1, h->q, h->w0);
  };
  once();
  once();
  FL_HIP(hipEventRecord(h->ev0, s));
  for (int a = 0; a < reps; ++a) once();
  FL_HIP(hipEventRecord(h->ev1, s));
  FL_HIP(hipStreamSynchronize(s));
  FL_HIP(hipGetLastError());
  float ms = 0.f;
  FL_HIP(hipEventElapsedTime(&ms, h->ev0, h->ev1));
  *ms_out = ms / reps;
  if (nblocks_out) *nblocks_out = plan.nblocks;
  return FL_SUCCESS;
}

// ------------------------------------------------------------------------------------------------ launch plans (tests/launch_regimes.py)
// Not part of the public C-ABI (not declared in fluca_hip.h): the launch shapes the hot kernels take on an nx x ny x nz block.  Host arithmetic
// only -- no handle, no HIP call.  Writes FLDBG_NPLAN ints to out (in this order) and returns their number; out == nullptr: the number only.
//   k_cg_A / k_cg_Bq (plan_cg_A):       0 ry, 1 nw, 2 tiles_x, 3 tiles_y, 4 nchunk, 5 zc, 6 nblocks
//   k_cheb2 (fl_cheb2_plan):            7 nw, 8 tiles_x, 9 tiles, 10 nchunk, 11 zc, 12 nblocks
//   k_apply_pc, k_bcgs_pw (tile_plan):  13 ry, 14 tiles_x, 15 nchunk, 16 zc, 17 nblocks
//   k_project_six (project_six_plan):   18 nxcd, 19 nseg, 20 nbx (blocks per XCD slab), 21 items (row segments per slab)
//   k_schur_var (schur_var_plan):       22 per_xcd, 23 nseg, 24 band, 25 fixed_seg, 26 items
//   k_mom2 / k_mom3 (mom_plan):         27 t2x, 28 t2chunk, 29 t2zc, 30 t2blocks
// Every field comes from the plan function the launcher itself calls.
constexpr int FLDBG_NPLAN = 31;
extern "C" int fldbg_launch_plans(int nx, int ny, int nz, int *out, int nout)
{
  if (nx < 1 || ny < 1 || nz < 1) return FL_ERR_ARG_OUTOFRANGE;
  if (!out) return FLDBG_NPLAN;
  if (nout < FLDBG_NPLAN) return FL_ERR_ARG_SIZ;
  GridP g{};
  g.nx = nx;
  g.ny = ny;
  g.nz = nz;
  const PlanA        a  = plan_cg_A(g, 0, 0);
  const Cheb2Plan    c  = fl_cheb2_plan(g);
  const TP           t  = tile_plan(g);
  const SchurVarPlan sv = schur_var_plan(g);
  const ProjectSixPlan p6 = project_six_plan(g);
  const MomPlan        m2 = mom_plan(g);
  if (p6.items > INT32_MAX || p6.nbx > INT32_MAX || sv.items > INT32_MAX) return FL_ERR_ARG_OUTOFRANGE;
  const int v[FLDBG_NPLAN] = {a.ry, a.nw, a.tiles_x, a.tiles_y, a.nchunk, a.zc, a.nblocks,
                              c.nw, c.tiles_x, c.tiles, c.nchunk, c.zc, c.nblocks,
                              t.ry, t.tiles_x, t.nchunk, t.zc, t.nblocks,
                              p6.nxcd, p6.nseg, (int)p6.nbx, (int)p6.items,
                              sv.per_xcd, sv.nseg, sv.band, sv.fixed_seg, (int)sv.items,
                              m2.t2x, m2.t2chunk, m2.t2zc, m2.t2blocks};
  std::memcpy(out, v, sizeof(v));
  return FLDBG_NPLAN;
}

// Not part of the public C-ABI either (tests/launch_regimes.py, rr.fused): 1 when a multigrid level of nx x ny x nz cells, halved on every axis,
// forms the coarse right-hand side with the one-pass residual + restriction (fl_residual_restrict_fusable, the shape test of
// fl_residual_restrict_padded), 0 when it runs the residual and k_mg_restrict.  Host arithmetic only.  A query of its own rather than a field of
// fldbg_launch_plans, whose count of FLDBG_NPLAN ints its callers check.
extern "C" int fldbg_mg_restrict_fused(int nx, int ny, int nz)
{
  if (nx < 1 || ny < 1 || nz < 1) return FL_ERR_ARG_OUTOFRANGE;
  GridP g{};
  g.nx = nx;
  g.ny = ny;
  g.nz = nz;
  return fl_residual_restrict_fusable(g) ? 1 : 0;
}


