/*
 * fluca_host.c -- C host mirror of Fluca's Mesh / NS plugin surface in front of the pressure-Poisson path
 * (include/fluca_host.h lists the reference interfaces).  Pure C99; reaches the GPU only through the C-ABI of
 * include/fluca_hip.h (libflucahip.so).  No PETSc, no MPI: one process per GPU, rank/size set explicitly.
 */
#include "../../include/fluca_host_impl.h"

#include <math.h>
#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <strings.h>

/* positive PETSC_ERR_* values */
enum { E_MEM = 55, E_SUP = 56, E_ARG_WRONG = 62, E_FILE_OPEN = 65, E_FILE_WRITE = 67 /* PETSC_ERR_FILE_WRITE (66 is FILE_READ) */, E_ARG_OUTOFRANGE = 63, E_ARG_WRONGSTATE = 73, E_ARG_NULL = 85, E_ARG_UNKNOWN_TYPE = 86, E_ARG_TYPENOTSET = 89 };

#define FLCHK(call)             \
  do {                          \
    FlErrorCode e_ = (call);    \
    if (e_) return e_;          \
  } while (0)
/* C-ABI calls return -(PETSC_ERR_*) */
#define FLABI(call)             \
  do {                          \
    int r_ = (call);            \
    if (r_) return -r_;         \
  } while (0)

/* the same inside a roctx range (trace_begin .. trace_end): the range is closed on the error path too */
#define FLABI_T(call)           \
  do {                          \
    int r_ = (call);            \
    if (r_) {                   \
      trace_end();              \
      return -r_;               \
    }                           \
  } while (0)
#define FLCHK_T(call)           \
  do {                          \
    FlErrorCode e_ = (call);    \
    if (e_) {                   \
      trace_end();              \
      return e_;                \
    }                           \
  } while (0)
static void trace_end(void);
static void trace_begin(const char *name);
/* FLUCA_STEP_TIMING=1: NSStep prints the wall time of its phases (each closed by a stream synchronise, so the sum is larger than an
 * untimed step): where a time step goes, without a profiler */
static int    step_timing(void);
static double step_clock(NS ns);
static FlErrorCode ns_jacobian(NS ns);
/* the bodies of the immersed boundary (NSSetImmersedBoundaryBodies) and the force monitor's context */
static FlErrorCode ibm_force_monitor_destroy(void **ctx);
static FlErrorCode ibm_body_to_ref(NS ns);
static FlErrorCode ibm_body_from_ref(NS ns, int64_t Ln);

/* ------------------------------------------------------------------------------------------------ registries */

#define MAXTYPES 16
typedef struct {
  char name[32];
  void *create;
} TypeEntry;
static TypeEntry MeshList[MAXTYPES], NSList[MAXTYPES];
static int       nMeshTypes = 0, nNSTypes = 0;
/* the type lists are the only process-wide state of this library: objects of several host threads (one rank each, tests/test_gpu_config5.py)
 * may reach MeshCreate / NSCreate together, so the built-in types are registered exactly once and the lists are appended to under a lock */
static pthread_once_t  register_once = PTHREAD_ONCE_INIT;
static pthread_mutex_t register_lock = PTHREAD_MUTEX_INITIALIZER;

static void RegisterBuiltins(void)
{
  MeshRegister(MESHCART, MeshCreate_Cart); /* meshreg.c */
  NSRegister(NSCNLINEAR, NSCreate_CNLinear); /* nsreg.c:17 */
}
static void RegisterAll(void) { pthread_once(&register_once, RegisterBuiltins); }

static const char *opt_find(int argc, char **argv, const char *name)
{
  for (int i = 1; i + 1 < argc; ++i)
    if (argv[i] && !strcmp(argv[i], name)) return argv[i + 1];
  return NULL;
}
/* PetscOptionsBool: a bare flag (last argument, or followed by another option) means true; otherwise the next token must be one of
 * true / false / yes / no / on / off / 1 / 0 (PetscOptionsStringToBool).  Returns 1 if the flag is present, -1 on a bad value. */
static int opt_flag(int argc, char **argv, const char *name, int *v)
{
  for (int i = 1; i < argc; ++i) {
    if (!argv[i] || strcmp(argv[i], name)) continue;
    const char *s = i + 1 < argc ? argv[i + 1] : NULL;
    if (!s || (s[0] == '-' && !(s[1] >= '0' && s[1] <= '9'))) {
      *v = 1;
      return 1;
    }
    if (!strcasecmp(s, "true") || !strcasecmp(s, "yes") || !strcasecmp(s, "on") || !strcmp(s, "1")) *v = 1;
    else if (!strcasecmp(s, "false") || !strcasecmp(s, "no") || !strcasecmp(s, "off") || !strcmp(s, "0")) *v = 0;
    else return -1;
    return 1;
  }
  return 0;
}
static int opt_int64(int argc, char **argv, const char *name, int64_t *v)
{
  const char *s = opt_find(argc, argv, name);
  if (!s) return 0;
  *v = strtoll(s, NULL, 10);
  return 1;
}
static int opt_real(int argc, char **argv, const char *name, double *v)
{
  const char *s = opt_find(argc, argv, name);
  if (!s) return 0;
  *v = strtod(s, NULL);
  return 1;
}

/* ------------------------------------------------------------------------------------------------ Viewer */

FlErrorCode FlucaViewerCreate(FlucaViewerType type, char mode, FlucaViewer *viewer)
{
  if (!type || !viewer) return E_ARG_NULL;
  FlucaViewer v = (FlucaViewer)calloc(1, sizeof(*v));
  if (!v) return E_MEM;
  v->type   = type;
  v->mode   = mode;
  v->seqnum = -1; /* meshbasic.c:25-26 */
  *viewer   = v;
  return 0;
}
static FlErrorCode ViewerVPrintf_ASCII(FlucaViewer v, const char *fmt, va_list ap)
{
  FILE *f = (FILE *)v->data;
  for (int i = 0; i < v->tab; ++i) fputs("  ", f); /* PetscViewerASCIIPrintf indents by two blanks per tab level */
  return vfprintf(f, fmt, ap) < 0 ? E_FILE_WRITE : 0;
}
static FlErrorCode ViewerDestroy_ASCII(FlucaViewer v)
{
  FILE *f = (FILE *)v->data;
  if (f && f != stdout) fclose(f);
  else if (f) fflush(f);
  return 0;
}
FlErrorCode FlucaViewerASCIIOpen(const char *filename, FlucaViewer *viewer)
{
  if (!viewer) return E_ARG_NULL;
  FILE *f = !filename || !strcmp(filename, "stdout") ? stdout : fopen(filename, "w");
  if (!f) return E_FILE_OPEN;
  const FlErrorCode rc = FlucaViewerCreate(FLUCAVIEWERASCII, 'w', viewer);
  if (rc) {
    if (f != stdout) fclose(f);
    return rc;
  }
  (*viewer)->data         = f;
  (*viewer)->ops->vprintf = ViewerVPrintf_ASCII;
  (*viewer)->ops->destroy = ViewerDestroy_ASCII;
  return 0;
}
FlErrorCode FlucaViewerASCIIPrintf(FlucaViewer viewer, const char *fmt, ...)
{
  if (!viewer || !fmt) return E_ARG_NULL;
  if (!viewer->ops->vprintf) return E_SUP;
  va_list ap;
  va_start(ap, fmt);
  const FlErrorCode rc = viewer->ops->vprintf(viewer, fmt, ap);
  va_end(ap);
  return rc;
}
FlErrorCode FlucaViewerASCIIPushTab(FlucaViewer viewer) { if (!viewer) return E_ARG_NULL; ++viewer->tab; return 0; }
FlErrorCode FlucaViewerASCIIPopTab(FlucaViewer viewer)
{
  if (!viewer) return E_ARG_NULL;
  if (viewer->tab <= 0) return E_ARG_WRONGSTATE; /* "More tabs popped than pushed" */
  --viewer->tab;
  return 0;
}
FlErrorCode FlucaViewerGetType(FlucaViewer viewer, FlucaViewerType *type)
{
  if (!viewer || !type) return E_ARG_NULL;
  *type = viewer->type;
  return 0;
}
FlErrorCode FlucaViewerDestroy(FlucaViewer *viewer)
{
  if (!viewer || !*viewer) return 0;
  const FlErrorCode rc = (*viewer)->ops->destroy ? (*viewer)->ops->destroy(*viewer) : 0;
  free(*viewer);
  *viewer = NULL;
  return rc;
}
static int viewer_is(FlucaViewer v, const char *type) { return v && v->type && !strcmp(v->type, type); }
/* viewer NULL = PetscViewerASCIIGetStdout: a stdout viewer for the length of the call */
#define WITH_STDOUT_VIEWER(viewer, body)                          \
  do {                                                            \
    FlucaViewer own_ = NULL;                                      \
    if (!(viewer)) {                                              \
      FLCHK(FlucaViewerASCIIOpen(NULL, &own_));                   \
      (viewer) = own_;                                            \
    }                                                             \
    FlErrorCode rc_ = (body);                                     \
    if (own_) FlucaViewerDestroy(&own_);                          \
    return rc_;                                                   \
  } while (0)

/* ------------------------------------------------------------------------------------------------ Mesh */

FlErrorCode MeshRegister(const char name[], FlErrorCode (*create)(Mesh))
{
  pthread_mutex_lock(&register_lock);
  if (nMeshTypes >= MAXTYPES) {
    pthread_mutex_unlock(&register_lock);
    return E_MEM;
  }
  snprintf(MeshList[nMeshTypes].name, sizeof(MeshList[0].name), "%s", name);
  MeshList[nMeshTypes].create = (void *)create;
  __atomic_store_n(&nMeshTypes, nMeshTypes + 1, __ATOMIC_RELEASE); /* readers (SetType) walk the list without the lock: the entry is complete before it counts */
  pthread_mutex_unlock(&register_lock);
  return 0;
}

FlErrorCode MeshCreate(Mesh *mesh)
{
  if (!mesh) return E_ARG_NULL;
  RegisterAll();
  Mesh m = (Mesh)calloc(1, sizeof(*m));
  if (!m) return E_MEM;
  m->dim  = 3;
  m->size = 1;
  *mesh   = m;
  return 0;
}

FlErrorCode MeshSetType(Mesh mesh, MeshType type)
{
  if (!mesh || !type) return E_ARG_NULL;
  for (int i = 0, nt = __atomic_load_n(&nMeshTypes, __ATOMIC_ACQUIRE); i < nt; ++i)
    if (!strcmp(MeshList[i].name, type)) {
      if (mesh->ops->destroy) FLCHK(mesh->ops->destroy(mesh));
      memset(mesh->ops, 0, sizeof(mesh->ops));
      snprintf(mesh->type_name, sizeof(mesh->type_name), "%s", type);
      return ((FlErrorCode(*)(Mesh))MeshList[i].create)(mesh);
    }
  return E_ARG_UNKNOWN_TYPE; /* "Unknown mesh type" */
}

FlErrorCode MeshSetRank(Mesh mesh, int rank, int size)
{
  if (!mesh) return E_ARG_NULL;
  if (mesh->setupcalled) return E_ARG_WRONGSTATE;
  if (size < 1 || rank < 0 || rank >= size) return E_ARG_OUTOFRANGE;
  mesh->rank = rank;
  mesh->size = size;
  return 0;
}

static FlErrorCode MeshSetFromOptions_Cart(Mesh mesh, int argc, char **argv)
{
  Mesh_Cart *cart = (Mesh_Cart *)mesh->data;
  char       opt[64];
  for (int d = 0; d < 3; ++d) { /* cart.c:21-36 */
    int64_t v;
    snprintf(opt, sizeof(opt), "-cart_grid_%c", 'x' + d);
    if (opt_int64(argc, argv, opt, &v)) {
      if (v < 1) return E_ARG_OUTOFRANGE;
      cart->N[d] = v;
    }
    snprintf(opt, sizeof(opt), "-cart_ranks_%c", 'x' + d);
    if (opt_int64(argc, argv, opt, &v)) cart->nRanks[d] = (int)v;
    snprintf(opt, sizeof(opt), "-cart_boundary_type_%c", 'x' + d);
    const char *s = opt_find(argc, argv, opt);
    if (s) {
      if (!strcasecmp(s, "none")) cart->bndTypes[d] = MESHCART_BOUNDARY_NONE;
      else if (!strcasecmp(s, "periodic")) cart->bndTypes[d] = MESHCART_BOUNDARY_PERIODIC;
      else return E_ARG_WRONG;
    }
    snprintf(opt, sizeof(opt), "-cart_refine_%c", 'x' + d); /* cart.c:37-41 */
    if (opt_int64(argc, argv, opt, &v)) {
      if (v < 1) return E_ARG_OUTOFRANGE;
      cart->refineFactor[d] = v;
    }
  }
  /* -cart_refine n: "Refine grid one or more times" (cart.c:42-52): the global sizes and any ownership ranges grow by
     refineFactor^n before the mesh is set up -- the reference's hook for a hierarchy of grids */
  int64_t nRefine = 0;
  if (opt_int64(argc, argv, "-cart_refine", &nRefine)) {
    if (nRefine < 0) return E_ARG_OUTOFRANGE;
    for (int d = 0; d < 3; ++d) {
      int64_t total = 1;
      for (int64_t i = 0; i < nRefine; ++i) total *= cart->refineFactor[d];
      cart->N[d] *= total;
      if (cart->l[d])
        for (int i = 0; i < cart->nRanks[d]; ++i) cart->l[d][i] *= total;
    }
  }
  return 0;
}

FlErrorCode MeshCartSetRefinementFactor(Mesh mesh, int64_t refine_x, int64_t refine_y, int64_t refine_z) /* cart.c:432-444 */
{
  if (!mesh) return E_ARG_NULL;
  if (mesh->setupcalled) return E_ARG_WRONGSTATE;
  Mesh_Cart *cart = (Mesh_Cart *)mesh->data;
  if (refine_x > 0) cart->refineFactor[0] = refine_x;
  if (refine_y > 0) cart->refineFactor[1] = refine_y;
  if (refine_z > 0) cart->refineFactor[2] = refine_z;
  return 0;
}
FlErrorCode MeshCartGetRefinementFactor(Mesh mesh, int64_t *refine_x, int64_t *refine_y, int64_t *refine_z) /* cart.c:446-456 */
{
  if (!mesh) return E_ARG_NULL;
  Mesh_Cart *cart = (Mesh_Cart *)mesh->data;
  if (refine_x) *refine_x = cart->refineFactor[0];
  if (refine_y) *refine_y = cart->refineFactor[1];
  if (refine_z) *refine_z = cart->refineFactor[2];
  return 0;
}

/* PETSC_DECIDE rank grid: like DMStag, as cubic as the factorisation of `size` allows, larger factors on longer axes */
static void decide_ranks(int size, const int64_t N[3], int ranks[3])
{
  int fixed = 1, nfree = 0;
  for (int d = 0; d < 3; ++d)
    if (ranks[d] > 0) fixed *= ranks[d];
    else ++nfree;
  int rest = size / (fixed > 0 ? fixed : 1);
  for (int d = 0; d < 3; ++d)
    if (ranks[d] <= 0) ranks[d] = 1;
  for (int f = 2; rest > 1;) {
    if (rest % f) {
      ++f;
      continue;
    }
    /* give the factor to the free axis with the most cells per rank */
    int best = -1;
    double bestv = -1.;
    for (int d = 2; d >= 0; --d) {
      (void)nfree;
      double v = (double)N[d] / ranks[d];
      if (v > bestv) {
        bestv = v;
        best  = d;
      }
    }
    ranks[best] *= f;
    rest /= f;
  }
}

static FlErrorCode MeshSetUp_Cart(Mesh mesh)
{
  Mesh_Cart *cart = (Mesh_Cart *)mesh->data;
  int        want[3] = {cart->nRanks[0], cart->nRanks[1], cart->nRanks[2]};
  decide_ranks(mesh->size, cart->N, want);
  if (want[0] * want[1] * want[2] != mesh->size) return E_ARG_WRONG; /* rank grid does not match the job size */
  for (int d = 0; d < 3; ++d) cart->nRanks[d] = want[d];
  FLABI(fl_decomp_default(cart->N, cart->nRanks, mesh->rank, &mesh->decomp));
  for (int d = 0; d < 3; ++d) {
    if (cart->l[d]) { /* user ownership ranges (MeshCartSetOwnershipRanges, cart.c:399-418) */
      int64_t lo = 0, sum = 0;
      for (int r = 0; r < cart->nRanks[d]; ++r) {
        if (r < mesh->decomp.coord[d]) lo += cart->l[d][r];
        sum += cart->l[d][r];
      }
      if (sum != cart->N[d]) return E_ARG_WRONG;
      mesh->decomp.lo[d]  = lo;
      mesh->decomp.len[d] = cart->l[d][mesh->decomp.coord[d]];
    } else {
      cart->l[d] = (int64_t *)malloc(sizeof(int64_t) * cart->nRanks[d]);
      for (int r = 0; r < cart->nRanks[d]; ++r) {
        int64_t q = cart->N[d] / cart->nRanks[d], rem = cart->N[d] % cart->nRanks[d];
        cart->l[d][r] = q + (r < rem ? 1 : 0);
      }
    }
  }
  mesh->setupcalled = 1;
  /* DMStagSetUniformCoordinatesProduct(sdm, 0, 1, 0, 1, 0, 1)  (cart.c:128) */
  FLCHK(MeshCartSetUniformCoordinates(mesh, 0., 1., 0., 1., 0., 1.));
  /* coordinates MeshLoad read replace the uniform ones axis by axis (cart.c:131-140) */
  for (int d = 0; d < 3; ++d)
    if (cart->coordLoaded[d]) {
      const int64_t n = cart->N[d];
      memcpy(cart->xf[d], cart->coordLoaded[d], sizeof(double) * (size_t)(n + 1));
      for (int64_t i = 0; i < n; ++i) cart->xc[d][i] = (cart->coordLoaded[d][i] + cart->coordLoaded[d][i + 1]) / 2.;
    }
  return 0;
}

static FlErrorCode MeshDestroy_Cart(Mesh mesh)
{
  Mesh_Cart *cart = (Mesh_Cart *)mesh->data;
  if (!cart) return 0;
  for (int d = 0; d < 3; ++d) {
    free(cart->l[d]);
    free(cart->xf[d]);
    free(cart->xc[d]);
    free(cart->coordLoaded[d]);
  }
  free(cart);
  mesh->data = NULL;
  return 0;
}

static FlErrorCode MeshGetNumberBoundaries_Cart(Mesh mesh, int *nb)
{
  *nb = 2 * mesh->dim;
  return 0;
}


/* cart.c:171-206 */
static FlErrorCode MeshView_Cart(Mesh mesh, FlucaViewer viewer)
{
  Mesh_Cart *cart = (Mesh_Cart *)mesh->data;
  if (viewer_is(viewer, FLUCAVIEWERASCII)) {
    if (!mesh->setupcalled) return E_ARG_WRONGSTATE; /* DMStagGetCorners on a DM that does not exist yet */
    const fl_decomp *D = &mesh->decomp;
    /* the reference prints cart->N[1] in the place of P (cart.c:193); the third size is meant and printed here */
    FLCHK(FlucaViewerASCIIPrintf(viewer, "Processor [%d] M %lld N %lld P %lld m %d n %d p %d\n", mesh->rank, (long long)cart->N[0], (long long)cart->N[1], (long long)cart->N[2],
                                 cart->nRanks[0], cart->nRanks[1], cart->nRanks[2]));
    FLCHK(FlucaViewerASCIIPrintf(viewer, "X range of indices: %lld %lld, Y range of indices: %lld %lld, Z range of indices: %lld %lld\n", (long long)D->lo[0], (long long)(D->lo[0] + D->len[0]),
                                 (long long)D->lo[1], (long long)(D->lo[1] + D->len[1]), (long long)D->lo[2], (long long)(D->lo[2] + D->len[2])));
    return 0;
  }
  if (viewer_is(viewer, FLUCAVIEWERCGNS)) {
    if (!mesh->setupcalled) return 0; /* cartcgns.c:14 */
    return viewer->ops->viewmesh ? viewer->ops->viewmesh(viewer, mesh) : E_SUP;
  }
  return 0;
}
/* cart.c:208-216 with cartcgns.c:120-158 */
static FlErrorCode MeshLoad_Cart(Mesh mesh, FlucaViewer viewer)
{
  Mesh_Cart *cart = (Mesh_Cart *)mesh->data;
  if (!viewer_is(viewer, FLUCAVIEWERCGNS)) return 0;
  if (!viewer->ops->loadmesh) return E_SUP;
  if (mesh->setupcalled) return E_ARG_WRONGSTATE; /* MeshCartSetGlobalSizes: "This function must be called before MeshSetUp()" */
  int64_t N[3];
  double *xf[3] = {NULL, NULL, NULL};
  FLCHK(viewer->ops->loadmesh(viewer, N, xf));
  for (int d = 0; d < 3; ++d) {
    free(cart->coordLoaded[d]);
    cart->coordLoaded[d] = xf[d];
    cart->N[d]           = N[d];
    cart->bndTypes[d]    = MESHCART_BOUNDARY_NONE; /* cartcgns.c:155 */
  }
  mesh->dim = 3;
  return 0;
}
/* cart.c:218-229: this rank's block of the DM as one zeroed device array */
static FlErrorCode MeshCreateGlobalVector_Cart(Mesh mesh, MeshDMType type, int device, double **vec, int64_t *n)
{
  if (!mesh->setupcalled) return E_ARG_WRONGSTATE;
  const fl_decomp *D = &mesh->decomp;
  Mesh_Cart       *cart = (Mesh_Cart *)mesh->data;
  const int64_t    cells = D->len[0] * D->len[1] * D->len[2];
  int64_t          faces = 0;
  for (int d = 0; d < 3; ++d) { /* DMStag ownership: the last rank of a non-periodic axis owns the extra face */
    const int extra = cart->bndTypes[d] != MESHCART_BOUNDARY_PERIODIC && D->coord[d] == D->ranks[d] - 1;
    faces += cells / D->len[d] * (D->len[d] + extra);
  }
  int64_t count;
  switch (type) {
  case MESH_DM_SCALAR: count = cells; break;
  case MESH_DM_VECTOR: count = 3 * cells; break;
  case MESH_DM_STAG_SCALAR: count = faces; break;
  case MESH_DM_STAG_VECTOR: count = 3 * faces; break;
  default: return E_ARG_OUTOFRANGE;
  }
  void *d = NULL;
  FLABI(fl_malloc(device, sizeof(double) * (size_t)(count > 0 ? count : 1), &d)); /* zero-initialised, like a fresh Vec */
  *vec = (double *)d;
  if (n) *n = count;
  return 0;
}

FlErrorCode MeshCreate_Cart(Mesh mesh) /* cart.c:262-288 */
{
  Mesh_Cart *cart = (Mesh_Cart *)calloc(1, sizeof(*cart));
  if (!cart) return E_MEM;
  for (int d = 0; d < 3; ++d) {
    cart->N[d]            = -1;
    cart->nRanks[d]       = FL_DECIDE;
    cart->refineFactor[d] = 2; /* cart.c:276 */
  }
  mesh->data                     = cart;
  mesh->ops->setfromoptions      = MeshSetFromOptions_Cart;
  mesh->ops->setup               = MeshSetUp_Cart;
  mesh->ops->destroy             = MeshDestroy_Cart;
  mesh->ops->view                = MeshView_Cart;
  mesh->ops->load                = MeshLoad_Cart;
  mesh->ops->createglobalvector  = MeshCreateGlobalVector_Cart;
  mesh->ops->creatematrix        = NULL; /* MeshCreateMatrix_Cart (cart.c:231-260) hands out AIJ matrices; nothing here is assembled */
  mesh->ops->getnumberboundaries = MeshGetNumberBoundaries_Cart;
  return 0;
}

FlErrorCode MeshCartCreate3d(MeshCartBoundaryType bndx, MeshCartBoundaryType bndy, MeshCartBoundaryType bndz, int64_t M, int64_t N, int64_t P, int m, int n, int p, const int64_t *lx, const int64_t *ly, const int64_t *lz, Mesh *mesh)
{
  FLCHK(MeshCreate(mesh));
  FLCHK(MeshSetType(*mesh, MESHCART));
  Mesh_Cart     *cart = (Mesh_Cart *)(*mesh)->data;
  const int64_t *l[3] = {lx, ly, lz};
  const int      r[3] = {m, n, p};
  cart->N[0] = M; cart->N[1] = N; cart->N[2] = P;
  cart->bndTypes[0] = bndx; cart->bndTypes[1] = bndy; cart->bndTypes[2] = bndz;
  for (int d = 0; d < 3; ++d) {
    cart->nRanks[d] = r[d];
    if (l[d]) {
      if (r[d] <= 0) return E_ARG_WRONGSTATE; /* "Cannot set ownership ranges before setting number of procs" */
      cart->l[d] = (int64_t *)malloc(sizeof(int64_t) * r[d]);
      memcpy(cart->l[d], l[d], sizeof(int64_t) * r[d]);
    }
  }
  return 0;
}

FlErrorCode MeshSetFromOptions(Mesh mesh, int argc, char **argv)
{
  if (!mesh) return E_ARG_NULL;
  if (mesh->setupcalled) return E_ARG_WRONGSTATE;
  if (!mesh->type_name[0]) FLCHK(MeshSetType(mesh, MESHCART));
  return mesh->ops->setfromoptions ? mesh->ops->setfromoptions(mesh, argc, argv) : 0;
}

FlErrorCode MeshSetUp(Mesh mesh)
{
  if (!mesh) return E_ARG_NULL;
  if (mesh->setupcalled) return 0;
  if (!mesh->type_name[0]) return E_ARG_TYPENOTSET;
  Mesh_Cart *cart = (Mesh_Cart *)mesh->data;
  for (int d = 0; d < 3; ++d)
    if (cart->N[d] < 1) return E_ARG_WRONGSTATE;
  return mesh->ops->setup(mesh);
}

FlErrorCode MeshCartSetUniformCoordinates(Mesh mesh, double xmin, double xmax, double ymin, double ymax, double zmin, double zmax)
{
  if (!mesh) return E_ARG_NULL;
  if (!mesh->setupcalled) return E_ARG_WRONGSTATE; /* "This function must be called after MeshSetUp()" cart.c:462 */
  Mesh_Cart   *cart = (Mesh_Cart *)mesh->data;
  const double lo[3] = {xmin, ymin, zmin}, hi[3] = {xmax, ymax, zmax};
  for (int d = 0; d < 3; ++d) {
    if (!(hi[d] > lo[d])) return E_ARG_WRONG;
    const int64_t n = cart->N[d];
    const double  h = (hi[d] - lo[d]) / (double)n;
    free(cart->xf[d]);
    free(cart->xc[d]);
    cart->xf[d] = (double *)malloc(sizeof(double) * (n + 1));
    cart->xc[d] = (double *)malloc(sizeof(double) * n);
    /* DMStagSetUniformCoordinatesProduct: prev = min + i h, element = min + (i + 1/2) h */
    for (int64_t i = 0; i <= n; ++i) cart->xf[d][i] = lo[d] + (double)i * h;
    for (int64_t i = 0; i < n; ++i) cart->xc[d][i] = lo[d] + ((double)i + 0.5) * h;
  }
  return 0;
}

FlErrorCode MeshCartSetCoordinates(Mesh mesh, const double *xf, const double *yf, const double *zf)
{
  if (!mesh || !xf || !yf || !zf) return E_ARG_NULL;
  if (!mesh->setupcalled) return E_ARG_WRONGSTATE;
  Mesh_Cart    *cart = (Mesh_Cart *)mesh->data;
  const double *in[3] = {xf, yf, zf};
  for (int d = 0; d < 3; ++d) {
    const int64_t n = cart->N[d];
    free(cart->xf[d]);
    free(cart->xc[d]);
    cart->xf[d] = (double *)malloc(sizeof(double) * (n + 1));
    cart->xc[d] = (double *)malloc(sizeof(double) * n);
    memcpy(cart->xf[d], in[d], sizeof(double) * (n + 1));
    for (int64_t i = 0; i < n; ++i) cart->xc[d][i] = (in[d][i] + in[d][i + 1]) / 2.; /* cart.c:136 */
  }
  return 0;
}

#define MESH_CART(mesh)                      \
  if (!(mesh)) return E_ARG_NULL;            \
  Mesh_Cart *cart = (Mesh_Cart *)(mesh)->data; \
  if (!cart) return E_ARG_TYPENOTSET

FlErrorCode MeshCartGetGlobalSizes(Mesh mesh, int64_t *M, int64_t *N, int64_t *P)
{
  MESH_CART(mesh);
  if (M) *M = cart->N[0];
  if (N) *N = cart->N[1];
  if (P) *P = cart->N[2];
  return 0;
}
FlErrorCode MeshCartGetNumRanks(Mesh mesh, int *m, int *n, int *p)
{
  MESH_CART(mesh);
  if (m) *m = cart->nRanks[0];
  if (n) *n = cart->nRanks[1];
  if (p) *p = cart->nRanks[2];
  return 0;
}
FlErrorCode MeshCartGetCorners(Mesh mesh, int64_t *x, int64_t *y, int64_t *z, int64_t *m, int64_t *n, int64_t *p)
{
  if (!mesh) return E_ARG_NULL;
  if (!mesh->setupcalled) return E_ARG_WRONGSTATE;
  const fl_decomp *d = &mesh->decomp;
  if (x) *x = d->lo[0];
  if (y) *y = d->lo[1];
  if (z) *z = d->lo[2];
  if (m) *m = d->len[0];
  if (n) *n = d->len[1];
  if (p) *p = d->len[2];
  return 0;
}
FlErrorCode MeshCartGetIsFirstRank(Mesh mesh, int *fx, int *fy, int *fz)
{
  if (!mesh) return E_ARG_NULL;
  if (!mesh->setupcalled) return E_ARG_WRONGSTATE;
  if (fx) *fx = mesh->decomp.coord[0] == 0;
  if (fy) *fy = mesh->decomp.coord[1] == 0;
  if (fz) *fz = mesh->decomp.coord[2] == 0;
  return 0;
}
FlErrorCode MeshCartGetIsLastRank(Mesh mesh, int *lx, int *ly, int *lz)
{
  if (!mesh) return E_ARG_NULL;
  if (!mesh->setupcalled) return E_ARG_WRONGSTATE;
  if (lx) *lx = mesh->decomp.coord[0] == mesh->decomp.ranks[0] - 1;
  if (ly) *ly = mesh->decomp.coord[1] == mesh->decomp.ranks[1] - 1;
  if (lz) *lz = mesh->decomp.coord[2] == mesh->decomp.ranks[2] - 1;
  return 0;
}
/* cart.c:467-510 MeshCartGetCoordinateArraysRead: borrowed GLOBAL face coordinates (n+1 per axis); nothing to restore */
FlErrorCode MeshCartGetCoordinateArraysRead(Mesh mesh, const double **xf, const double **yf, const double **zf)
{
  if (!mesh) return E_ARG_NULL;
  if (!mesh->setupcalled) return E_ARG_WRONGSTATE;
  Mesh_Cart *cart = (Mesh_Cart *)mesh->data;
  if (xf) *xf = cart->xf[0];
  if (yf) *yf = cart->xf[1];
  if (zf) *zf = cart->xf[2];
  return 0;
}
FlErrorCode MeshGetRank(Mesh mesh, int *rank, int *size)
{
  if (!mesh) return E_ARG_NULL;
  if (rank) *rank = mesh->rank;
  if (size) *size = mesh->size;
  return 0;
}
FlErrorCode MeshCartGetBoundaryIndex(Mesh mesh, MeshCartBoundaryLocation loc, int *index)
{
  if (!mesh || !index) return E_ARG_NULL;
  if ((int)loc < 0 || (int)loc > 5) return E_ARG_WRONG; /* "Invalid boundary location" cart.c:587 */
  *index = (int)loc;                                     /* LEFT 0, RIGHT 1, DOWN 2, UP 3, BACK 4, FRONT 5  cart.c:568-586 */
  return 0;
}
FlErrorCode MeshGetNumberBoundaries(Mesh mesh, int *nb)
{
  if (!mesh || !nb) return E_ARG_NULL;
  if (!mesh->ops->getnumberboundaries) return E_ARG_TYPENOTSET;
  return mesh->ops->getnumberboundaries(mesh, nb);
}
static FlErrorCode MeshView_Body(Mesh mesh, FlucaViewer viewer)
{
  if (viewer_is(viewer, FLUCAVIEWERASCII)) /* PetscObjectPrintClassNamePrefixType */
    FLCHK(FlucaViewerASCIIPrintf(viewer, "Mesh Object: %d MPI process%s\n  type: %s\n", mesh->size, mesh->size > 1 ? "es" : "", mesh->type_name[0] ? mesh->type_name : "not yet set"));
  if (mesh->ops->view) FLCHK(mesh->ops->view(mesh, viewer)); /* PetscTryTypeMethod */
  return 0;
}
FlErrorCode MeshView(Mesh mesh, FlucaViewer viewer) /* meshbasic.c:93-104 */
{
  if (!mesh) return E_ARG_NULL;
  WITH_STDOUT_VIEWER(viewer, MeshView_Body(mesh, viewer));
}
FlErrorCode MeshLoad(Mesh mesh, FlucaViewer viewer) /* meshbasic.c:114-127 */
{
  if (!mesh || !viewer) return E_ARG_NULL;
  if (viewer->mode != 'r') return E_ARG_WRONGSTATE; /* PetscViewerCheckReadable */
  if (!viewer_is(viewer, FLUCAVIEWERCGNS)) return E_ARG_WRONG; /* "Invalid viewer; open viewer with PetscViewerFlucaCGNSOpen()" */
  if (!mesh->type_name[0]) FLCHK(MeshSetType(mesh, MESHCART));
  if (!mesh->ops->load) return E_SUP; /* PetscUseTypeMethod */
  return mesh->ops->load(mesh, viewer);
}
FlErrorCode MeshCreateGlobalVector(Mesh mesh, MeshDMType type, int device, double **vec_dev, int64_t *n)
{
  if (!mesh || !vec_dev) return E_ARG_NULL;
  if (!mesh->ops->createglobalvector) return E_SUP;
  return mesh->ops->createglobalvector(mesh, type, device, vec_dev, n);
}
FlErrorCode MeshCreateMatrix(Mesh mesh, MeshDMType rtype, MeshDMType ctype, void **mat)
{
  if (!mesh || !mat) return E_ARG_NULL;
  if (!mesh->ops->creatematrix) return E_SUP; /* matrix-free build: no type assembles a Mat */
  return mesh->ops->creatematrix(mesh, rtype, ctype, mat);
}
FlErrorCode MeshDestroy(Mesh *mesh)
{
  if (!mesh || !*mesh) return 0;
  if ((*mesh)->ops->destroy) (*mesh)->ops->destroy(*mesh);
  free(*mesh);
  *mesh = NULL;
  return 0;
}

/* ------------------------------------------------------------------------------------------------ NS */

FlErrorCode NSRegister(const char name[], FlErrorCode (*create)(NS))
{
  pthread_mutex_lock(&register_lock);
  if (nNSTypes >= MAXTYPES) {
    pthread_mutex_unlock(&register_lock);
    return E_MEM;
  }
  snprintf(NSList[nNSTypes].name, sizeof(NSList[0].name), "%s", name);
  NSList[nNSTypes].create = (void *)create;
  __atomic_store_n(&nNSTypes, nNSTypes + 1, __ATOMIC_RELEASE); /* readers (SetType) walk the list without the lock: the entry is complete before it counts */
  pthread_mutex_unlock(&register_lock);
  return 0;
}

FlErrorCode NSCreate(NS *ns)
{
  if (!ns) return E_ARG_NULL;
  RegisterAll();
  NS n = (NS)calloc(1, sizeof(*n));
  if (!n) return E_MEM;
  n->rho = 1.; /* nsbasic.c:31-35 defaults */
  n->mu  = 1.;
  n->dt  = 0.;
  n->max_steps = -1;
  n->max_time  = 1.7976931348623157e308;
  n->errorifstepfailed = 1;
  n->scalar_stages = 5; /* the reference's -ts_type ssp default */
  n->scalar_theta  = 0.;
  n->scalar_rtol   = 1e-6;
  n->scalar_implicit_ranks = 0;
  n->scalar_ibm_passes = 1;
  n->bc_keep           = 1;
  fl_ksp_opts_default(&n->schur);
  fl_ksp_opts_default(&n->mom);
  n->mom.type = FL_KSP_BCGS; /* PETSc's own default for kspA is gmres + ilu: neither has a matrix-free form here */
  n->mom.pc   = FL_PC_JACOBI;
  n->mom.remove_nullspace = 0;
  n->ksp_type   = 2;
  n->gmres_restart = 30;
  n->ksp_rtol   = 1e-5; /* nssol.c:24 */
  n->ksp_atol   = 1e-50;
  n->ksp_max_it = 10000;
  *ns = n;
  return 0;
}

FlErrorCode NSSetType(NS ns, NSType type)
{
  if (!ns || !type) return E_ARG_NULL;
  for (int i = 0, nt = __atomic_load_n(&nNSTypes, __ATOMIC_ACQUIRE); i < nt; ++i)
    if (!strcmp(NSList[i].name, type)) {
      if (ns->ops->destroy) FLCHK(ns->ops->destroy(ns));
      memset(ns->ops, 0, sizeof(ns->ops));
      snprintf(ns->type_name, sizeof(ns->type_name), "%s", type);
      return ((FlErrorCode(*)(NS))NSList[i].create)(ns);
    }
  return E_ARG_UNKNOWN_TYPE;
}
FlErrorCode NSGetType(NS ns, NSType *type)
{
  if (!ns || !type) return E_ARG_NULL;
  *type = ns->type_name[0] ? ns->type_name : NULL;
  return 0;
}

FlErrorCode NSSetMesh(NS ns, Mesh mesh)
{
  if (!ns || !mesh) return E_ARG_NULL;
  if (ns->setupcalled) return E_ARG_WRONGSTATE;
  int nb;
  FLCHK(MeshGetNumberBoundaries(mesh, &nb));
  free(ns->bcs);
  ns->bcs  = (NSBoundaryCondition *)calloc((size_t)nb, sizeof(NSBoundaryCondition)); /* all NS_BC_NONE, nsopts.c:19-22 */
  ns->nb   = nb;
  ns->mesh = mesh;
  return 0;
}
FlErrorCode NSSetDevice(NS ns, int device)
{
  if (!ns) return E_ARG_NULL;
  if (ns->setupcalled) return E_ARG_WRONGSTATE;
  ns->device = device;
  return 0;
}
FlErrorCode NSSetDensity(NS ns, double rho)
{
  if (!ns) return E_ARG_NULL;
  if (!(rho > 0.)) return E_ARG_OUTOFRANGE;
  ns->rho = rho;
  return 0;
}
FlErrorCode NSSetViscosity(NS ns, double mu)
{
  if (!ns) return E_ARG_NULL;
  if (!(mu > 0.)) return E_ARG_OUTOFRANGE;
  ns->mu = mu;
  return 0;
}
FlErrorCode NSSetTimeStepSize(NS ns, double dt)
{
  if (!ns) return E_ARG_NULL;
  if (!(dt > 0.)) return E_ARG_OUTOFRANGE;
  ns->dt = dt;
  return 0;
}
FlErrorCode NSSetMaxTime(NS ns, double max_time) /* nsopts.c:111-117 */
{
  if (!ns) return E_ARG_NULL;
  ns->max_time = max_time;
  return 0;
}
FlErrorCode NSGetMaxTime(NS ns, double *max_time)
{
  if (!ns) return E_ARG_NULL;
  if (max_time) *max_time = ns->max_time;
  return 0;
}
FlErrorCode NSSetMaxSteps(NS ns, int64_t max_steps)
{
  if (!ns) return E_ARG_NULL;
  ns->max_steps = max_steps;
  return 0;
}
FlErrorCode NSSetBoundaryCondition(NS ns, int index, NSBoundaryCondition bc)
{
  if (!ns) return E_ARG_NULL;
  if (!ns->mesh) return E_ARG_WRONGSTATE; /* "Mesh not set" */
  if (index < 0 || index >= ns->nb) return E_ARG_OUTOFRANGE;
  ns->bcs[index] = bc;
  /* the kept boundary planes of this boundary were evaluated with the condition that is being replaced (same function and context pointers are no
   * proof of the same values: a caller may have changed what ctx points to and say so by setting the condition again) */
  if (ns->data && !strcmp(ns->type_name, NSCNLINEAR)) {
    NS_CNLinear *c = (NS_CNLinear *)ns->data;
    if (index < 6) c->bc_have[index][0] = c->bc_have[index][1] = 0;
  }
  return 0;
}
FlErrorCode NSGetBoundaryCondition(NS ns, int index, NSBoundaryCondition *bc)
{
  if (!ns || !bc) return E_ARG_NULL;
  if (index < 0 || index >= ns->nb) return E_ARG_OUTOFRANGE;
  *bc = ns->bcs[index];
  return 0;
}

FlErrorCode NSSetFromOptions(NS ns, int argc, char **argv)
{
  if (!ns) return E_ARG_NULL;
  const char *s;
  double      v;
  int64_t     iv;
  if ((s = opt_find(argc, argv, "-ns_type"))) FLCHK(NSSetType(ns, s));
  if (!ns->type_name[0]) FLCHK(NSSetType(ns, NSCNLINEAR));
  if (opt_real(argc, argv, "-ns_density", &v)) FLCHK(NSSetDensity(ns, v)); /* nsopts.c:180-186 */
  if (opt_real(argc, argv, "-ns_viscosity", &v)) FLCHK(NSSetViscosity(ns, v));
  if (opt_real(argc, argv, "-ns_time_step_size", &v)) FLCHK(NSSetTimeStepSize(ns, v));
  if (opt_int64(argc, argv, "-ns_max_steps", &iv)) ns->max_steps = iv;
  if (opt_real(argc, argv, "-ns_max_time", &v)) ns->max_time = v; /* nsopts.c:186 */
  {
    int flg = 0;
    const int got = opt_flag(argc, argv, "-ns_error_if_step_failed", &flg); /* :188 */
    if (got < 0) return E_ARG_WRONG;
    if (got) ns->errorifstepfailed = flg;
  }
  {
    int flg = 0;
    const int got = opt_flag(argc, argv, "-ns_keep_boundary_values", &flg); /* mirror only: see fluca_host.h */
    if (got < 0) return E_ARG_WRONG;
    if (got) ns->bc_keep = flg;
  }
  /* mirror only: how NSSetImmersedBoundary holds the markers on several ranks.  replicated (default): every rank keeps all of them, the
   * interpolation ends in an all-reduce.  owner: every rank keeps the markers of its block and ghost copies of its neighbours' (fl_ibm_create_owned).
   * A user's choice for now: which one is faster is decided by the latency between GPUs, and nothing has been measured on two GPUs yet. */
  if ((s = opt_find(argc, argv, "-ns_ibm_marker_distribution"))) {
    if (!strcmp(s, "replicated")) ns->ibm_owner = 0;
    else if (!strcmp(s, "owner")) ns->ibm_owner = 1;
    else return E_ARG_UNKNOWN_TYPE;
  }
  /* passive scalars (NSAddScalar): the limiter of a scalar added without one, the stages of the SSP step */
  if ((s = opt_find(argc, argv, "-ns_scalar_limiter"))) {
    int l = 0;
    if (fl_limiter_from_name(s, &l)) return E_ARG_UNKNOWN_TYPE;
    ns->scalar_limiter = l;
  }
  if (opt_int64(argc, argv, "-ns_scalar_stages", &iv)) {
    if (iv < 2 || iv > 1000) return E_ARG_OUTOFRANGE;
    ns->scalar_stages = (int)iv;
  }
  /* mirror only: implicit diffusion of the scalars added from here on (NSSetScalarImplicit): theta 0 (explicit) or in [0.5, 1], rtol in (0, 1) */
  if (opt_real(argc, argv, "-ns_scalar_implicit_theta", &v)) {
    if (!(v == 0. || (v >= 0.5 && v <= 1.))) return E_ARG_OUTOFRANGE;
    ns->scalar_theta = v;
  }
  if (opt_real(argc, argv, "-ns_scalar_implicit_rtol", &v)) {
    if (!(v > 0. && v < 1.)) return E_ARG_OUTOFRANGE;
    ns->scalar_rtol = v;
  }
  /* ... and whether the two options above also reach scalars added on a several-rank mesh (NSSetScalarImplicitRanks; default 0: they stay explicit there) */
  if (opt_int64(argc, argv, "-ns_scalar_implicit_ranks", &iv)) {
    if (iv < 0 || iv > 1) return E_ARG_OUTOFRANGE;
    ns->scalar_implicit_ranks = (int)iv;
  }
  /* mirror only: the passes NSSetScalarImmersedBoundary(npass = -1) takes */
  if (opt_int64(argc, argv, "-ns_scalar_ibm_passes", &iv)) {
    if (iv < 1 || iv > 16) return E_ARG_OUTOFRANGE;
    ns->scalar_ibm_passes = (int)iv;
  }
  /* mirror only: gravity of the Boussinesq term (NSSetGravity), three numbers separated by commas */
  if ((s = opt_find(argc, argv, "-ns_gravity"))) {
    double g[3];
    int    k = 0;
    for (const char *q = s; k < 3; ++k) {
      char *end;
      g[k] = strtod(q, &end);
      if (end == q || *end != (k < 2 ? ',' : '\0')) return E_ARG_WRONG;
      q = end + 1;
    }
    FLCHK(NSSetGravity(ns, g));
  }
  /* mirror only: force and torque on the immersed bodies, one line per step and body (NSMonitorImmersedBoundaryForce) */
  if ((s = opt_find(argc, argv, "-ns_ibm_force_monitor"))) {
    char *name = strdup(s);
    if (!name) return E_MEM;
    const FlErrorCode e = NSMonitorSet(ns, NSMonitorImmersedBoundaryForce, name, ibm_force_monitor_destroy);
    if (e) {
      free(name);
      return e;
    }
  }
  /* sub-KSP of the Schur complement: prefix ns_ + abf_schur_ (nssol.c:19, abfpc.c:206) */
  if ((s = opt_find(argc, argv, "-ns_abf_schur_ksp_type"))) {
    if (!strcmp(s, "cg")) ns->schur.type = FL_KSP_CG;
    else if (!strcmp(s, "bcgs")) ns->schur.type = FL_KSP_BCGS;
    else if (!strcmp(s, "chebyshev")) ns->schur.type = FL_KSP_CHEBYSHEV;
    else return E_ARG_UNKNOWN_TYPE; /* PETSc: "Unable to find requested KSP type" */
  }
  if ((s = opt_find(argc, argv, "-ns_abf_schur_pc_type"))) {
    if (!strcmp(s, "jacobi")) ns->schur.pc = FL_PC_JACOBI;
    else if (!strcmp(s, "none")) ns->schur.pc = FL_PC_NONE;
    else if (!strcmp(s, "mg")) ns->schur.pc = FL_PC_MG; /* geometric multigrid of fl_mg.hip (KSPCG only) */
    else return E_ARG_UNKNOWN_TYPE;
  }
  if (opt_int64(argc, argv, "-ns_abf_schur_pc_mg_levels", &iv)) ns->schur.mg_levels = (int)iv;
  if (opt_int64(argc, argv, "-ns_abf_schur_mg_levels_ksp_max_it", &iv)) ns->schur.mg_smooth_its = (int)iv;
  if ((s = opt_find(argc, argv, "-ns_abf_schur_ksp_norm_type"))) {
    if (!strcmp(s, "preconditioned")) ns->schur.norm_type = FL_NORM_PRECONDITIONED;
    else if (!strcmp(s, "unpreconditioned")) ns->schur.norm_type = FL_NORM_UNPRECONDITIONED;
    else if (!strcmp(s, "natural")) ns->schur.norm_type = FL_NORM_NATURAL;
    else if (!strcmp(s, "none")) ns->schur.norm_type = FL_NORM_NONE;
    else return E_ARG_UNKNOWN_TYPE;
  }
  if (opt_real(argc, argv, "-ns_abf_schur_ksp_rtol", &v)) ns->schur.rtol = v;
  if (opt_real(argc, argv, "-ns_abf_schur_ksp_atol", &v)) ns->schur.atol = v;
  if (opt_real(argc, argv, "-ns_abf_schur_ksp_divtol", &v)) ns->schur.dtol = v;
  if (opt_int64(argc, argv, "-ns_abf_schur_ksp_max_it", &iv)) ns->schur.maxit = (int)iv;
  {
    int flg = 0;
    const int got = opt_flag(argc, argv, "-ns_abf_schur_ksp_cg_single_reduction", &flg);
    if (got < 0) return E_ARG_WRONG; /* "Unknown logical value" */
    if (got) ns->schur.cg_single_reduction = flg;
  }
  if ((s = opt_find(argc, argv, "-ns_abf_schur_ksp_chebyshev_eigenvalues"))) {
    if (sscanf(s, "%lf,%lf", &ns->schur.emin, &ns->schur.emax) != 2) return E_ARG_WRONG;
  }
  /* the outer KSP of ns->snes (nssol.c:21-29): prefix ns_ */
  if ((s = opt_find(argc, argv, "-ns_ksp_type"))) {
    if (!strcmp(s, "richardson")) ns->ksp_type = 0;
    else if (!strcmp(s, "preonly")) ns->ksp_type = 1;
    else if (!strcmp(s, "gmres")) ns->ksp_type = 2;
    else return !strcmp(s, "fgmres") || !strcmp(s, "bcgs") ? E_SUP : E_ARG_UNKNOWN_TYPE;
  }
  if (opt_int64(argc, argv, "-ns_ksp_gmres_restart", &iv)) {
    if (iv < 1 || iv > 200) return E_ARG_OUTOFRANGE;
    ns->gmres_restart = (int)iv;
  }
  if (opt_real(argc, argv, "-ns_ksp_rtol", &v)) ns->ksp_rtol = v;
  if (opt_real(argc, argv, "-ns_ksp_atol", &v)) ns->ksp_atol = v;
  if (opt_int64(argc, argv, "-ns_ksp_max_it", &iv)) ns->ksp_max_it = (int)iv;
  /* sub-KSP of the momentum block: prefix ns_ + abf_momentum_ (abfpc.c:205) */
  if ((s = opt_find(argc, argv, "-ns_abf_momentum_ksp_type"))) {
    if (!strcmp(s, "bcgs")) ns->mom.type = FL_KSP_BCGS;
    else if (!strcmp(s, "gmres")) ns->mom.type = FL_KSP_GMRES; /* the reference's own default type of kspA (abfpc.c:72) */
    else if (!strcmp(s, "chebyshev")) ns->mom.type = FL_KSP_CHEBYSHEV; /* KSPCHEBYSHEV fused into the product; interval below or from the Gershgorin disc */
    else return !strcmp(s, "cg") || !strcmp(s, "fgmres") ? E_SUP : E_ARG_UNKNOWN_TYPE;
  }
  if (opt_int64(argc, argv, "-ns_abf_momentum_ksp_gmres_restart", &iv)) {
    if (iv < 1 || iv > 1000) return E_ARG_OUTOFRANGE;
    ns->mom.gmres_restart = (int)iv;
  }
  if ((s = opt_find(argc, argv, "-ns_abf_momentum_pc_type"))) {
    if (!strcmp(s, "jacobi")) ns->mom.pc = FL_PC_JACOBI;
    else if (!strcmp(s, "none")) ns->mom.pc = FL_PC_NONE;
    else return !strcmp(s, "ilu") || !strcmp(s, "bjacobi") ? E_SUP : E_ARG_UNKNOWN_TYPE;
  }
  if ((s = opt_find(argc, argv, "-ns_abf_momentum_ksp_chebyshev_eigenvalues"))) {
    if (sscanf(s, "%lf,%lf", &ns->mom.emin, &ns->mom.emax) != 2) return E_ARG_WRONG;
  }
  if ((s = opt_find(argc, argv, "-ns_abf_momentum_ksp_norm_type"))) {
    if (!strcmp(s, "preconditioned")) ns->mom.norm_type = FL_NORM_PRECONDITIONED;
    else if (!strcmp(s, "unpreconditioned")) ns->mom.norm_type = FL_NORM_UNPRECONDITIONED;
    else if (!strcmp(s, "none")) ns->mom.norm_type = FL_NORM_NONE;
    else return !strcmp(s, "natural") ? E_SUP : E_ARG_UNKNOWN_TYPE;
  }
  {
    /* mirror only: the first PCApply_ABF of a time step starts kspA from the previous velocity (VecCopy(v0, v*) + KSPSetInitialGuessNonzero in front of
     * abfpc.c:72); the other applications of the step (Richardson corrections) start from zero.  Same convergence test against || M momrhs ||. */
    int flg = 0;
    const int got = opt_flag(argc, argv, "-ns_abf_momentum_guess_previous", &flg);
    if (got < 0) return E_ARG_WRONG;
    if (got) ns->mom_guess_previous = flg;
    /* ... or from the velocity extrapolated through the two previous steps, 2 v^n - v^(n-1) (the first step: v^n) */
    const int got2 = opt_flag(argc, argv, "-ns_abf_momentum_guess_extrapolate", &flg);
    if (got2 < 0) return E_ARG_WRONG;
    if (got2 && flg) ns->mom_guess_previous = 2;
  }
  if (opt_real(argc, argv, "-ns_abf_momentum_ksp_rtol", &v)) ns->mom.rtol = v;
  if (opt_real(argc, argv, "-ns_abf_momentum_ksp_atol", &v)) ns->mom.atol = v;
  if (opt_real(argc, argv, "-ns_abf_momentum_ksp_divtol", &v)) ns->mom.dtol = v;
  if (opt_int64(argc, argv, "-ns_abf_momentum_ksp_max_it", &iv)) ns->mom.maxit = (int)iv;
  /* PCABFAinvType of the Schur complement and of the upper-triangular solve (abfpc.c:246-247; PetscOptionsEnum matches the
   * names without regard to case) */
  {
    const char *names[2] = {"-ns_pc_abf_schur_ainv_type", "-ns_pc_abf_upper_ainv_type"};
    int        *dst[2]   = {&ns->schur_ainv, &ns->upper_ainv};
    for (int q = 0; q < 2; ++q)
      if ((s = opt_find(argc, argv, names[q]))) {
        if (!strcasecmp(s, "ID")) *dst[q] = FL_ABF_AINV_ID;
        else if (!strcasecmp(s, "DIAG")) *dst[q] = FL_ABF_AINV_DIAG;
        else if (!strcasecmp(s, "ROWSUM")) *dst[q] = FL_ABF_AINV_ROWSUM;
        else return E_ARG_UNKNOWN_TYPE;
      }
    if (ns->momentum) FLABI(fl_abf_set_ainv_types(ns->momentum, ns->schur_ainv, ns->upper_ainv));
  }
  return ns->ops->setfromoptions ? ns->ops->setfromoptions(ns, argc, argv) : 0;
}

/* Tracing: roctx ranges with the names of the reference's PetscLogEvents (nspkg.c:21-24: NSSetUp, NSStep, NSFormJacobian,
 * NSFormFunction), so that a rocprofv3 --marker-trace timeline reads like the reference's -log_view.  libroctx64 is looked up at
 * run time; without it the ranges are no-ops. */
#include <dlfcn.h>
static int (*roctx_push)(const char *) = NULL;
static int (*roctx_pop)(void)          = NULL;
static pthread_once_t trace_once = PTHREAD_ONCE_INIT;
static void trace_load(void)
{
  void *lib = dlopen("libroctx64.so", RTLD_NOW | RTLD_GLOBAL);
  if (!lib) lib = dlopen("libroctx64.so.4", RTLD_NOW | RTLD_GLOBAL);
  if (!lib) lib = dlopen("/opt/rocm/lib/libroctx64.so", RTLD_NOW | RTLD_GLOBAL);
  if (!lib) return;
  int (*push)(const char *) = (int (*)(const char *))dlsym(lib, "roctxRangePushA");
  int (*pop)(void)          = (int (*)(void))dlsym(lib, "roctxRangePop");
  if (push && pop) {
    roctx_pop  = pop;
    roctx_push = push; /* last: trace_begin tests this one */
  }
}
static void trace_init(void) { pthread_once(&trace_once, trace_load); }
static void trace_begin(const char *name)
{
  trace_init();
  if (roctx_push) (void)roctx_push(name);
}
static void trace_end(void)
{
  if (roctx_pop) (void)roctx_pop();
}
FlErrorCode FlucaTraceEnabled(void)
{
  trace_init();
  return roctx_push != NULL;
}

static FlErrorCode NSSetUp_Body(NS ns) /* nsbasic.c:153-274, restricted to what the Poisson path needs */
{
  if (!ns) return E_ARG_NULL;
  if (ns->setupcalled) return 0;
  if (!ns->type_name[0]) FLCHK(NSSetType(ns, NSCNLINEAR)); /* "Set default type" */
  if (!ns->mesh) return E_ARG_WRONGSTATE;                   /* "Mesh not set" */
  if (!ns->mesh->setupcalled) return E_ARG_WRONGSTATE;
  if (!(ns->dt > 0.)) return E_ARG_WRONGSTATE;
  Mesh_Cart *cart = (Mesh_Cart *)ns->mesh->data;
  int        bc[6], needs = 1;
  for (int b = 0; b < 6; ++b) {
    bc[b] = (int)ns->bcs[b].type;
    /* the mesh's periodic axes and the NS periodic BCs must agree */
    if ((cart->bndTypes[b / 2] == MESHCART_BOUNDARY_PERIODIC) != (ns->bcs[b].type == NS_BC_PERIODIC)) return E_ARG_WRONG;
    switch (ns->bcs[b].type) { /* nsbasic.c:217-231 */
    case NS_BC_VELOCITY:
    case NS_BC_PERIODIC:
    case NS_BC_SYMMETRY: break;
    case NS_BC_PRESSURE_OUTLET: needs = 0; break;
    default: return E_SUP; /* "Unsupported boundary condition type" */
    }
  }
  ns->schur.remove_nullspace = needs;
  fl_grid g;
  for (int d = 0; d < 3; ++d) {
    g.n[d]  = cart->N[d];
    g.xf[d] = cart->xf[d];
    g.xc[d] = cart->xc[d];
  }
  FLABI(fl_poisson_create(&g, bc, ns->dt / ns->rho, ns->mesh->size > 1 ? &ns->mesh->decomp : NULL, ns->device, &ns->poisson));
  /* "Create Jacobian" + "Initialize Jacobian" (nsbasic.c:203-207): NSFormJacobian(ns, ns->x = NULL, ns->J, NS_INIT_JACOBIAN) through the
   * type's slot.  A block too small for the momentum rows (fewer than two cells along an axis) has no J: the pressure path
   * (NSPressureCorrection) still works there and NSStep reports PETSC_ERR_SUP. */
  {
    const int rc = fl_momentum_create(ns->poisson, &ns->momentum);
    if (rc && rc != FL_ERR_SUP) return -rc;
    if (rc) ns->momentum = NULL;
    else if (ns->ops->formjacobian) FLCHK(NSFormJacobian(ns, NULL, ns->momentum, NS_INIT_JACOBIAN));
  }
  if (ns->ops->setup) FLCHK(ns->ops->setup(ns));
  ns->setupcalled = 1;
  return 0;
}

static FlErrorCode ibm_move(NS ns);
static FlErrorCode scalars_step(NS ns);
static int         buoyancy_active(NS ns);

static FlErrorCode NSStep_Body(NS ns) /* nsbasic.c:276-299 */
{
  if (!ns) return E_ARG_NULL;
  if (!ns->setupcalled) return E_ARG_WRONGSTATE;
  if (!ns->ops->step) return E_SUP;
  if (ns->ibm && ns->ibm_motion) FLCHK(ibm_move(ns)); /* the body in prescribed motion at t + dt, before the forcing term is formed */
  FLCHK(ns->ops->step(ns)); /* VecCopy(sol, sol0) + the type's step */
  if (ns->reason >= 0 && ns->nscalar) FLCHK(scalars_step(ns)); /* every passive scalar over dt in the new V */
  if (ns->reason >= 0) {
    ++ns->step;
    ns->t += ns->dt;
  }
  ns->ibm_force_ready = ns->ibm != NULL && ns->reason >= 0; /* ibm_U holds this step's U_target - interp(v0): NSGetImmersedBoundaryForce */
  if (ns->reason < 0 && ns->errorifstepfailed) { /* :293-297 */
    NSMonitorCancel(ns);
    return 91; /* PETSC_ERR_NOT_CONVERGED: "NSStep has failed due to DIVERGED_NONLINEAR_SOLVE" */
  }
  return 0;
}

/* nsbasic.c:301-323 */
FlErrorCode NSFormJacobian(NS ns, const NSVec *x, NSMat J, NSFormJacobianType type)
{
  if (!ns || !J) return E_ARG_NULL;
  if (!ns->ops->formjacobian) return E_SUP; /* PetscUseTypeMethod: "No method formjacobian for NS of type ..." */
  trace_begin("NSFormJacobian");
  const FlErrorCode rc = ns->ops->formjacobian(ns, x, J, type);
  trace_end();
  return rc;
}
FlErrorCode NSFormFunction(NS ns, const NSVec *x, NSVec *f)
{
  if (!ns || !f) return E_ARG_NULL;
  if (!ns->ops->formfunction) return E_SUP;
  trace_begin("NSFormFunction");
  const FlErrorCode rc = ns->ops->formfunction(ns, x, f);
  trace_end();
  return rc;
}
FlErrorCode NSGetJacobian(NS ns, NSMat *J)
{
  if (!ns || !J) return E_ARG_NULL;
  if (!ns->setupcalled) return E_ARG_WRONGSTATE;
  FLCHK(ns_jacobian(ns));
  *J = ns->momentum;
  return 0;
}

static FlErrorCode NSView_Body(NS ns, FlucaViewer viewer) /* nsbasic.c:353-374 */
{
  if (!viewer_is(viewer, FLUCAVIEWERASCII)) return 0;
  FLCHK(FlucaViewerASCIIPrintf(viewer, "NS Object: %d MPI process%s\n  type: %s\n", ns->mesh ? ns->mesh->size : 1, ns->mesh && ns->mesh->size > 1 ? "es" : "",
                               ns->type_name[0] ? ns->type_name : "not yet set")); /* PetscObjectPrintClassNamePrefixType */
  FLCHK(FlucaViewerASCIIPrintf(viewer, "Density: %g, Viscosity: %g, Time step size: %g\n", ns->rho, ns->mu, ns->dt));
  FLCHK(FlucaViewerASCIIPrintf(viewer, "Current time step: %d, Current time: %g\n", (int)ns->step, ns->t));
  FLCHK(FlucaViewerASCIIPushTab(viewer));
  const FlErrorCode rc = ns->ops->view ? ns->ops->view(ns, viewer) : 0; /* PetscTryTypeMethod */
  if (!rc && buoyancy_active(ns)) { /* mirror only, and only while the term is there: the output without it is the reference's */
    FLCHK(FlucaViewerASCIIPrintf(viewer, "Gravity: (%g, %g, %g)\n", ns->gravity[0], ns->gravity[1], ns->gravity[2]));
    for (int a = 0; a < ns->nscalar; ++a)
      if (ns->scalars[a].beta != 0.)
        FLCHK(FlucaViewerASCIIPrintf(viewer, "Buoyant scalar %s: beta %g, reference %g\n", ns->scalars[a].name, ns->scalars[a].beta, ns->scalars[a].phi_ref));
  }
  for (int a = 0; !rc && a < ns->nscalar; ++a) /* mirror only, and only while the forcing is on */
    if (ns->scalars[a].ibm_npass > 0 && ns->ibm) {
      char   vals[64 * 32];
      size_t at = 0;
      vals[0]   = 0;
      for (int b = 0; b < (ns->ibm_nbody ? ns->ibm_nbody : 1) && at + 32 < sizeof(vals); ++b) at += (size_t)snprintf(vals + at, 32, " %g", ns->scalars[a].ibm_value[b]);
      FLCHK(FlucaViewerASCIIPrintf(viewer, "Scalar %s on the immersed boundary: %d pass%s, value%s\n", ns->scalars[a].name, ns->scalars[a].ibm_npass, ns->scalars[a].ibm_npass == 1 ? "" : "es", vals));
    }
  FLCHK(FlucaViewerASCIIPopTab(viewer));
  return rc;
}
FlErrorCode NSView(NS ns, FlucaViewer viewer)
{
  if (!ns) return E_ARG_NULL;
  WITH_STDOUT_VIEWER(viewer, NSView_Body(ns, viewer));
}

/* nssol.c:130-150.  The three field links of NSSetUp (nsbasic.c:180-182) in their order, then the type's own vectors. */
static FlErrorCode NSViewSolution_Body(NS ns, FlucaViewer viewer)
{
  if (!ns->setupcalled) return E_ARG_WRONGSTATE;
  if (viewer->mode != 'w') return E_ARG_WRONGSTATE;
  if (viewer_is(viewer, FLUCAVIEWERASCII)) {
    /* nssol.c:130-150 VecViews each field on whatever viewer it is given; an ASCII dump of 10^8 numbers serves nobody, so the ASCII viewer gets
     * what VecView prints first -- the field names and their sizes -- and the numbers go to a CGNS viewer */
    int64_t sz[4];
    FLCHK(NSGetLocalSizes(ns, sz));
    FLCHK(FlucaViewerASCIIPrintf(viewer, "NS solution at step %lld, time %g:\n", (long long)ns->step, ns->t));
    FLCHK(FlucaViewerASCIIPrintf(viewer, "  Velocity: 3 x %lld cell values\n  FaceNormalVelocity: %lld + %lld + %lld face values\n  Pressure: %lld cell values\n", (long long)sz[0],
                                 (long long)sz[1], (long long)sz[2], (long long)sz[3], (long long)sz[0]));
    if (ns->ops->viewsolution && !strcmp(ns->type_name, NSCNLINEAR)) FLCHK(FlucaViewerASCIIPrintf(viewer, "  PressureHalfStep: %lld cell values\n", (long long)sz[0]));
    return 0;
  }
  if (!viewer->ops->solutionbegin || !viewer->ops->cellfield || !viewer->ops->facefield || !viewer->ops->solutionend) return E_SUP;
  double *v, *V[3], *p;
  FLCHK(NSGetSolutionArrays(ns, &v, V, &p));
  FLCHK(viewer->ops->solutionbegin(viewer, ns, 1));
  FLCHK(viewer->ops->cellfield(viewer, ns, "Velocity", 3, v));
  FLCHK(viewer->ops->facefield(viewer, ns, "FaceNormalVelocity", V));
  FLCHK(viewer->ops->cellfield(viewer, ns, "Pressure", 1, p));
  if (ns->ops->viewsolution) FLCHK(ns->ops->viewsolution(ns, viewer)); /* PetscTryTypeMethod(ns, viewsolution, viewer) */
  return viewer->ops->solutionend(viewer, ns);
}
FlErrorCode NSViewSolution(NS ns, FlucaViewer viewer) /* viewer NULL = PetscViewerASCIIGetStdout, as in the reference (nssol.c:136-137) */
{
  if (!ns) return E_ARG_NULL;
  WITH_STDOUT_VIEWER(viewer, NSViewSolution_Body(ns, viewer));
}
/* nssol.c:174-203 */
FlErrorCode NSLoadSolution(NS ns, FlucaViewer viewer)
{
  if (!ns || !viewer) return E_ARG_NULL;
  if (!ns->setupcalled) return E_ARG_WRONGSTATE; /* "This function must be called after NSSetUp()" */
  if (viewer->mode != 'r') return E_ARG_WRONGSTATE; /* PetscViewerCheckReadable */
  if (!viewer->ops->solutionbegin || !viewer->ops->cellfield || !viewer->ops->facefield || !viewer->ops->solutionend) return E_SUP;
  if (!ns->ops->loadsolution) return E_SUP; /* PetscUseTypeMethod(ns, loadsolution, viewer): checked before anything is read into ns->sol */
  double *v, *V[3], *p;
  FLCHK(NSGetSolutionArrays(ns, &v, V, &p));
  viewer->seqnum = -1; /* MeshSetOutputSequenceNumber(ns->mesh, -1, 0.): "reset here and will be set in VecLoad()" */
  viewer->seqval = 0.;
  FLCHK(viewer->ops->solutionbegin(viewer, ns, 0));
  FLCHK(viewer->ops->cellfield(viewer, ns, "Velocity", 3, v));
  FLCHK(viewer->ops->facefield(viewer, ns, "FaceNormalVelocity", V));
  FLCHK(viewer->ops->cellfield(viewer, ns, "Pressure", 1, p));
  FLCHK(ns->ops->loadsolution(ns, viewer));
  FLCHK(viewer->ops->solutionend(viewer, ns));
  if (viewer->seqnum < 0) return 76; /* PETSC_ERR_LIB: the file held no solution */
  ns->step = viewer->seqnum; /* MeshGetOutputSequenceNumber, nssol.c:199-201 */
  ns->t    = viewer->seqval;
  return 0;
}

FlErrorCode NSSetUp(NS ns)
{
  trace_begin("NSSetUp"); /* PetscLogEventBegin(NS_SetUp), nsbasic.c:160 */
  const FlErrorCode rc = NSSetUp_Body(ns);
  trace_end();
  return rc;
}
FlErrorCode NSStep(NS ns)
{
  trace_begin("NSStep"); /* PetscLogEventBegin(NS_Step), nsbasic.c:283 */
  const FlErrorCode rc = NSStep_Body(ns);
  trace_end();
  return rc;
}

/* nsopts.c: the plain getters / setters */
FlErrorCode NSGetDensity(NS ns, double *rho) { if (!ns || !rho) return E_ARG_NULL; *rho = ns->rho; return 0; }
FlErrorCode NSGetViscosity(NS ns, double *mu) { if (!ns || !mu) return E_ARG_NULL; *mu = ns->mu; return 0; }
FlErrorCode NSGetTimeStepSize(NS ns, double *dt) { if (!ns || !dt) return E_ARG_NULL; *dt = ns->dt; return 0; }
FlErrorCode NSGetMaxSteps(NS ns, int64_t *max_steps) { if (!ns || !max_steps) return E_ARG_NULL; *max_steps = ns->max_steps; return 0; }
FlErrorCode NSSetTime(NS ns, double t) { if (!ns) return E_ARG_NULL; ns->t = t; return 0; }
FlErrorCode NSSetTimeStep(NS ns, int64_t step) { if (!ns) return E_ARG_NULL; if (step < 0) return E_ARG_OUTOFRANGE; ns->step = step; return 0; }
FlErrorCode NSSetErrorIfStepFailed(NS ns, int flg) { if (!ns) return E_ARG_NULL; ns->errorifstepfailed = flg != 0; return 0; }
FlErrorCode NSGetErrorIfStepFailed(NS ns, int *flg) { if (!ns || !flg) return E_ARG_NULL; *flg = ns->errorifstepfailed; return 0; }
/* NSConvergedReason (flucans.h:13-18): 0 ITERATING, 1 CONVERGED_TIME, 2 CONVERGED_ITS, -1 DIVERGED_NONLINEAR_SOLVE */
FlErrorCode NSGetConvergedReason(NS ns, int *reason)
{
  if (!ns || !reason) return E_ARG_NULL;
  if (ns->reason < 0) *reason = -1;
  else if (ns->max_steps >= 0 && ns->step >= ns->max_steps) *reason = 2;
  else if (ns->t >= ns->max_time) *reason = 1;
  else *reason = 0;
  return 0;
}

/* nsmon.c:5-45: NSMonitorSet / NSMonitorCancel / NSMonitor */
FlErrorCode NSMonitorSet(NS ns, FlErrorCode (*mon)(NS, void *), void *ctx, FlErrorCode (*destroy)(void **))
{
  if (!ns || !mon) return E_ARG_NULL;
  if (ns->nmon >= MAXNSMONITORS) return E_ARG_OUTOFRANGE; /* "Too many monitors set" */
  ns->mon[ns->nmon]        = mon;
  ns->monctx[ns->nmon]     = ctx;
  ns->mondestroy[ns->nmon] = destroy;
  ++ns->nmon;
  return 0;
}
FlErrorCode NSMonitorCancel(NS ns)
{
  if (!ns) return E_ARG_NULL;
  for (int i = 0; i < ns->nmon; ++i)
    if (ns->mondestroy[i]) FLCHK(ns->mondestroy[i](&ns->monctx[i]));
  ns->nmon = 0;
  return 0;
}
FlErrorCode NSMonitor(NS ns)
{
  if (!ns) return E_ARG_NULL;
  for (int i = 0; i < ns->nmon; ++i) FLCHK(ns->mon[i](ns, ns->monctx[i]));
  return 0;
}

FlErrorCode NSSolve(NS ns) /* nsbasic.c:325-350: monitor, step, ... until -ns_max_steps or -ns_max_time, monitor once more */
{
  if (!ns) return E_ARG_NULL;
  if (ns->max_steps < 0 && !(ns->max_time < 1.7976931348623157e308)) return E_ARG_WRONGSTATE; /* "At least one of max time or max steps must be specified" */
  const int64_t max_steps = ns->max_steps < 0 ? INT64_MAX : ns->max_steps;
  while (ns->step < max_steps && ns->t < ns->max_time) { /* NS_CONVERGED_ITS, else NS_CONVERGED_TIME (:333-334, :342-343) */
    FLCHK(NSMonitor(ns));
    FLCHK(NSStep(ns));
    if (ns->reason < 0) break; /* with -ns_error_if_step_failed 0: NS_DIVERGED_NONLINEAR_SOLVE ends the loop (:337-345) */
  }
  FLCHK(NSMonitor(ns));
  return 0;
}

FlErrorCode NSGetInnerIterations(NS ns, int *momentum_its, int *schur_its)
{
  if (!ns) return E_ARG_NULL;
  if (momentum_its) *momentum_its = ns->mom_its;
  if (schur_its) *schur_its = ns->schur_its;
  return 0;
}

FlErrorCode NSGetLinearSolveInfo(NS ns, int *its, double *rnorm, int *reason)
{
  if (!ns) return E_ARG_NULL;
  if (its) *its = ns->ksp_its;
  if (rnorm) *rnorm = ns->ksp_rnorm;
  if (reason) *reason = ns->reason;
  return 0;
}
FlErrorCode NSGetLinearSolveResidualNorms(NS ns, double *rnorm0, double *rnorm)
{
  if (!ns) return E_ARG_NULL;
  if (rnorm0) *rnorm0 = ns->ksp_rnorm0;
  if (rnorm) *rnorm = ns->ksp_rnorm;
  return 0;
}
FlErrorCode NSGetTimeStep(NS ns, int64_t *step)
{
  if (!ns || !step) return E_ARG_NULL;
  *step = ns->step;
  return 0;
}
FlErrorCode NSGetTime(NS ns, double *t)
{
  if (!ns || !t) return E_ARG_NULL;
  *t = ns->t;
  return 0;
}

static void ibm_free_own(NS ns);

/* ---- passive scalars (fluca_host.h) */
#define MAXNSSCALARS 8
#define NS_SCALAR_CHEB_MAXIT 100000 /* far beyond any count the bound asks for: 1e-12 at a diffusion number of 1e6 takes under 30000 steps */
static FlErrorCode scalar_get(NS ns, int id, struct NSScalar **sc)
{
  if (!ns) return E_ARG_NULL;
  if (!ns->setupcalled) return E_ARG_WRONGSTATE;
  if (id < 0 || id >= ns->nscalar) return E_ARG_OUTOFRANGE;
  *sc = &ns->scalars[id];
  return 0;
}
/* the handle, created with the boundary types as they stand and given the solution's face velocities */
static FlErrorCode scalar_ensure(NS ns, struct NSScalar *sc)
{
  if (!sc->h) {
    FLABI(fl_scalar_create_ranks(ns->poisson, sc->kind, &sc->h)); /* collective on a several-rank mesh; one rank: fl_scalar_create */
    FLABI(fl_scalar_set_limiter(sc->h, sc->limiter));
    FLABI(fl_scalar_set_diffusivity(sc->h, sc->gamma));
    for (int b = 0; b < 6; ++b) FLABI(fl_scalar_set_boundary_value(sc->h, b, sc->val[b]));
  }
  double *V[3];
  FLCHK(NSGetSolutionArrays(ns, NULL, V, NULL));
  FLABI(fl_scalar_set_velocity(sc->h, V[0], V[1], V[2]));
  return 0;
}
/* NSSetScalarImmersedBoundary: phi to the bodies' values on the markers as they stand, and what that hands to the fluid into the step's sums */
static FlErrorCode scalar_ibm_force(NS ns, struct NSScalar *sc)
{
  const int64_t  L     = ns->ibm_L;
  const int      nbody = ns->ibm_nbody ? ns->ibm_nbody : 1;
  const int32_t *body  = ns->ibm_nbody ? ns->ibm_body : NULL;
  if (!ns->ibm_Q || L > ns->ibm_Qcap) { /* the first use, or a migration has brought more markers than ever */
    void *q = NULL;
    FLABI(fl_poisson_synchronize(ns->poisson));
    if (ns->ibm_Q) fl_free(ns->device, ns->ibm_Q);
    ns->ibm_Q = NULL;
    FLABI(fl_malloc(ns->device, sizeof(double) * (size_t)(L + L / 4 + 1), &q));
    ns->ibm_Q    = (double *)q;
    ns->ibm_Qcap = L + L / 4;
  }
  double r[64];
  FLABI(fl_ibm_scalar_force(ns->ibm, sc->ibm_npass, NULL, body, nbody, sc->ibm_value, L > 0 ? ns->ibm_dV : NULL, sc->phi, ns->ibm_Q));
  FLABI(fl_ibm_scalar_rate(ns->ibm, L > 0 ? ns->ibm_Q : NULL, L > 0 ? ns->ibm_dV : NULL, body, nbody, r));
  for (int b = 0; b < nbody; ++b) sc->ibm_sum[b] += r[b];
  return 0;
}
static FlErrorCode scalars_step(NS ns)
{
  for (int a = 0; a < ns->nscalar; ++a) {
    struct NSScalar *sc = &ns->scalars[a];
    FLCHK(scalar_ensure(ns, sc));
    const int forced = sc->ibm_npass > 0 && ns->ibm;
    if (forced) {
      sc->ibm_sum_ready = 0;
      for (int b = 0; b < 64; ++b) sc->ibm_sum[b] = 0.;
    }
    if (sc->theta == 0.) {
      for (int k = 0; k < sc->substeps; ++k) {
        FLABI(fl_scalar_step(sc->h, ns->dt / sc->substeps, ns->scalar_stages, sc->src, sc->phi));
        if (forced) FLCHK(scalar_ibm_force(ns, sc));
      }
      if (forced) sc->ibm_sum_ready = 1, sc->ibm_sum_dt = ns->dt;
      continue;
    }
    /* implicit diffusion (NSSetScalarImplicit): the stages without the diffusion term, then a fixed number of Chebyshev launches -- nothing waits.  On a
     * several-rank mesh (NSSetScalarImplicitRanks) the collective call: one plane of phi across every rank face per Chebyshev launch, still no reduction */
    for (int k = 0; k < sc->substeps; ++k) {
      fl_scalar_cheb_info info;
      if (ns->mesh->size > 1)
        FLABI(fl_scalar_step_imex_ranks(sc->h, ns->dt / sc->substeps, ns->scalar_stages, sc->theta, sc->rtol, NS_SCALAR_CHEB_MAXIT, sc->src, sc->phi, &info));
      else
        FLABI(fl_scalar_step_imex(sc->h, ns->dt / sc->substeps, ns->scalar_stages, sc->theta, sc->rtol, NS_SCALAR_CHEB_MAXIT, sc->src, sc->phi, &info));
      sc->cheb_steps = info.steps;
      sc->cheb_bound = info.bound;
      if (forced) FLCHK(scalar_ibm_force(ns, sc));
    }
    if (forced) sc->ibm_sum_ready = 1, sc->ibm_sum_dt = ns->dt;
  }
  return 0;
}
/* a new marker set or new bodies: the values held no longer say which body they belong to */
static void scalars_ibm_off(NS ns)
{
  for (int a = 0; a < ns->nscalar; ++a) ns->scalars[a].ibm_npass = ns->scalars[a].ibm_sum_ready = 0;
}
FlErrorCode NSSetScalarImmersedBoundary(NS ns, int id, int npass, const double *value)
{
  struct NSScalar *sc = NULL;
  if (!ns) return E_ARG_NULL;
  if (npass < -1 || npass > 16) return E_ARG_OUTOFRANGE;
  if (!ns->setupcalled || !ns->ibm) return E_ARG_WRONGSTATE;
  FLCHK(scalar_get(ns, id, &sc));
  if (npass == -1) npass = ns->scalar_ibm_passes;
  if (npass > 0 && !value) return E_ARG_NULL;
  const int nbody = ns->ibm_nbody ? ns->ibm_nbody : 1;
  for (int b = 0; b < nbody && npass > 0; ++b)
    if (!(value[b] - value[b] == 0.)) return E_ARG_OUTOFRANGE;
  for (int b = 0; b < 64; ++b) sc->ibm_value[b] = (npass > 0 && b < nbody) ? value[b] : 0.;
  sc->ibm_npass     = npass;
  sc->ibm_sum_ready = 0;
  return 0;
}
FlErrorCode NSGetScalarImmersedBoundaryRate(NS ns, int id, double *rate)
{
  struct NSScalar *sc = NULL;
  if (!ns || !rate) return E_ARG_NULL;
  if (!ns->setupcalled || !ns->ibm) return E_ARG_WRONGSTATE;
  FLCHK(scalar_get(ns, id, &sc));
  if (sc->ibm_npass == 0 || !sc->ibm_sum_ready || !(sc->ibm_sum_dt > 0.)) return E_ARG_WRONGSTATE;
  const int nbody = ns->ibm_nbody ? ns->ibm_nbody : 1;
  for (int b = 0; b < nbody; ++b) rate[b] = (1. / sc->ibm_sum_dt) * sc->ibm_sum[b];
  return 0;
}
FlErrorCode NSAddScalar(NS ns, const char *name, double gamma, const char *limiter_name, int *id)
{
  if (!ns || !name || !id) return E_ARG_NULL;
  if (!ns->setupcalled) return E_ARG_WRONGSTATE;
  if (!(gamma >= 0.) || gamma > 1.7976931348623157e308 || strlen(name) > 31 || ns->nscalar >= MAXNSSCALARS) return E_ARG_OUTOFRANGE;
  int limiter = ns->scalar_limiter;
  if (limiter_name && fl_limiter_from_name(limiter_name, &limiter)) return E_ARG_UNKNOWN_TYPE;
  if (!ns->scalars && !(ns->scalars = (struct NSScalar *)calloc(MAXNSSCALARS, sizeof(struct NSScalar)))) return E_MEM;
  struct NSScalar *sc = &ns->scalars[ns->nscalar];
  memset(sc, 0, sizeof(*sc));
  strcpy(sc->name, name);
  sc->gamma    = gamma;
  sc->limiter  = limiter;
  sc->substeps = 1;
  /* (several ranks: the option applies with -ns_scalar_implicit_ranks 1 alone, as NSSetScalarImplicit says E_SUP there and NSSetScalarImplicitRanks does not) */
  sc->theta    = (ns->mesh->size > 1 && !ns->scalar_implicit_ranks) ? 0. : ns->scalar_theta;
  sc->rtol     = ns->scalar_rtol;
  sc->cheb_bound = 1.;
  Mesh_Cart *cart = (Mesh_Cart *)ns->mesh->data;
  for (int b = 0; b < 6; ++b) sc->kind[b] = cart->bndTypes[b / 2] == MESHCART_BOUNDARY_PERIODIC ? 2 : 1;
  int64_t sz[4];
  FLABI(fl_poisson_sizes(ns->poisson, sz));
  void *zero = calloc((size_t)sz[0], sizeof(double));
  if (!zero) return E_MEM;
  int rc = fl_malloc(ns->device, sizeof(double) * (size_t)sz[0], (void **)&sc->phi);
  if (!rc) rc = fl_memcpy_h2d(ns->device, sc->phi, zero, sizeof(double) * (size_t)sz[0]);
  free(zero);
  if (rc) {
    if (sc->phi) fl_free(ns->device, sc->phi);
    sc->phi = NULL;
    return -rc;
  }
  *id = ns->nscalar++;
  return 0;
}
FlErrorCode NSSetScalarBoundaryCondition(NS ns, int id, int index, int type, double value)
{
  struct NSScalar *sc = NULL;
  FLCHK(scalar_get(ns, id, &sc));
  if (index < 0 || index > 5 || type < 0 || type > 2 || !(value - value == 0.)) return E_ARG_OUTOFRANGE;
  if (sc->h && sc->kind[index] != type) { /* the types are the handle's: a new one with the next use */
    FLABI(fl_scalar_destroy(sc->h));
    sc->h = NULL;
  }
  sc->kind[index] = type;
  sc->val[index]  = value;
  if (sc->h) FLABI(fl_scalar_set_boundary_value(sc->h, index, value));
  return 0;
}
FlErrorCode NSSetScalarSource(NS ns, int id, const double *src_dev)
{
  struct NSScalar *sc = NULL;
  FLCHK(scalar_get(ns, id, &sc));
  sc->src = src_dev;
  return 0;
}
FlErrorCode NSSetScalarSubsteps(NS ns, int id, int n)
{
  struct NSScalar *sc = NULL;
  FLCHK(scalar_get(ns, id, &sc));
  if (n < 1) return E_ARG_OUTOFRANGE;
  sc->substeps = n;
  return 0;
}
FlErrorCode NSSetScalarImplicit(NS ns, int id, double theta, double rtol)
{
  struct NSScalar *sc = NULL;
  FLCHK(scalar_get(ns, id, &sc));
  if (!(theta == 0. || (theta >= 0.5 && theta <= 1.)) || !(rtol > 0. && rtol < 1.)) return E_ARG_OUTOFRANGE;
  if (theta != 0. && ns->mesh->size > 1) return E_SUP; /* fl_scalar_step_imex runs on one rank */
  sc->theta = theta;
  sc->rtol  = rtol;
  return 0;
}
FlErrorCode NSSetScalarImplicitRanks(NS ns, int id, double theta, double rtol)
{
  struct NSScalar *sc = NULL;
  FLCHK(scalar_get(ns, id, &sc));
  if (!(theta == 0. || (theta >= 0.5 && theta <= 1.)) || !(rtol > 0. && rtol < 1.)) return E_ARG_OUTOFRANGE;
  sc->theta = theta; /* (any mesh: NSStep takes fl_scalar_step_imex_ranks on several ranks) */
  sc->rtol  = rtol;
  return 0;
}
FlErrorCode NSGetScalarImplicitInfo(NS ns, int id, int *steps, double *bound)
{
  struct NSScalar *sc = NULL;
  if (!steps || !bound) return E_ARG_NULL;
  FLCHK(scalar_get(ns, id, &sc));
  *steps = sc->cheb_steps;
  *bound = sc->cheb_bound;
  return 0;
}
FlErrorCode NSGetScalarArray(NS ns, int id, double **phi_dev)
{
  struct NSScalar *sc = NULL;
  if (!phi_dev) return E_ARG_NULL;
  FLCHK(scalar_get(ns, id, &sc));
  *phi_dev = sc->phi;
  return 0;
}
FlErrorCode NSGetScalarCFL(NS ns, int id, double out[2])
{
  struct NSScalar *sc = NULL;
  if (!out) return E_ARG_NULL;
  FLCHK(scalar_get(ns, id, &sc));
  FLCHK(scalar_ensure(ns, sc));
  FLABI(fl_scalar_cfl(sc->h, ns->dt / sc->substeps, out));
  return 0;
}
FlErrorCode NSGetScalarBoundaryFlux(NS ns, int id, double out[12])
{
  struct NSScalar *sc = NULL;
  if (!out) return E_ARG_NULL;
  FLCHK(scalar_get(ns, id, &sc));
  FLCHK(scalar_ensure(ns, sc));
  FLABI(fl_scalar_boundary_flux(sc->h, sc->phi, out));
  return 0;
}

/* ---- scalars that drive the flow: the Boussinesq term (fluca_host.h) */
FlErrorCode NSSetGravity(NS ns, const double g[3])
{
  if (!ns || !g) return E_ARG_NULL;
  for (int d = 0; d < 3; ++d)
    if (!(g[d] - g[d] == 0.)) return E_ARG_OUTOFRANGE;
  for (int d = 0; d < 3; ++d) ns->gravity[d] = g[d];
  return 0;
}
FlErrorCode NSGetGravity(NS ns, double g[3])
{
  if (!ns || !g) return E_ARG_NULL;
  for (int d = 0; d < 3; ++d) g[d] = ns->gravity[d];
  return 0;
}
FlErrorCode NSSetScalarBuoyancy(NS ns, int id, double beta, double phi_ref)
{
  struct NSScalar *sc = NULL;
  FLCHK(scalar_get(ns, id, &sc));
  if (!(beta - beta == 0.) || !(phi_ref - phi_ref == 0.)) return E_ARG_OUTOFRANGE;
  sc->beta    = beta;
  sc->phi_ref = phi_ref;
  return 0;
}
/* the term is there: gravity is not zero and some scalar has beta != 0 */
static int buoyancy_active(NS ns)
{
  if (ns->gravity[0] == 0. && ns->gravity[1] == 0. && ns->gravity[2] == 0.) return 0;
  for (int a = 0; a < ns->nscalar; ++a)
    if (ns->scalars[a].beta != 0.) return 1;
  return 0;
}
/* momrhs += dt sum_s (-beta_s g) (phi_s - phi_ref_s) over the scalars with beta != 0, in the order of their ids: one launch, or none */
static FlErrorCode buoyancy_add(NS ns, double *momrhs)
{
  if (!buoyancy_active(ns)) return 0;
  const double *phi[MAXNSSCALARS];
  double        accel[3 * MAXNSSCALARS], ref[MAXNSSCALARS];
  int           n = 0;
  for (int a = 0; a < ns->nscalar; ++a) {
    const struct NSScalar *sc = &ns->scalars[a];
    if (sc->beta == 0.) continue;
    phi[n] = sc->phi;
    ref[n] = sc->phi_ref;
    for (int d = 0; d < 3; ++d) accel[3 * n + d] = -sc->beta * ns->gravity[d];
    ++n;
  }
  FLABI(fl_momentum_add_buoyancy(ns->momentum, n, phi, accel, ref, ns->dt, momrhs));
  return 0;
}

FlErrorCode NSDestroy(NS *ns)
{
  if (!ns || !*ns) return 0;
  NSMonitorCancel(*ns);
  for (int a = 0; a < (*ns)->nscalar; ++a) { /* before the type's data and the Poisson handle they borrow */
    if ((*ns)->scalars[a].h) fl_scalar_destroy((*ns)->scalars[a].h);
    if ((*ns)->scalars[a].phi) fl_free((*ns)->device, (*ns)->scalars[a].phi);
  }
  free((*ns)->scalars);
  if ((*ns)->ops->destroy) (*ns)->ops->destroy(*ns);
  if ((*ns)->ibm) fl_ibm_destroy((*ns)->ibm);
  if ((*ns)->ibm_U) fl_free((*ns)->device, (*ns)->ibm_U);
  if ((*ns)->ibm_Q) fl_free((*ns)->device, (*ns)->ibm_Q);
  ibm_free_own(*ns);
  if ((*ns)->momentum) fl_momentum_destroy((*ns)->momentum);
  if ((*ns)->poisson) fl_poisson_destroy((*ns)->poisson);
  free((*ns)->bcs);
  free(*ns);
  *ns = NULL;
  return 0;
}

FlErrorCode NSGetPoisson(NS ns, fl_poisson **poisson)
{
  if (!ns || !poisson) return E_ARG_NULL;
  if (!ns->setupcalled) return E_ARG_WRONGSTATE;
  *poisson = ns->poisson;
  return 0;
}
FlErrorCode NSGetSchurKSPOptions(NS ns, fl_ksp_opts **opts)
{
  if (!ns || !opts) return E_ARG_NULL;
  *opts = &ns->schur;
  return 0;
}
FlErrorCode NSGetNeedsNullSpace(NS ns, int *needs)
{
  if (!ns || !needs) return E_ARG_NULL;
  if (!ns->setupcalled) return E_ARG_WRONGSTATE;
  *needs = ns->schur.remove_nullspace;
  return 0;
}
FlErrorCode NSGetLocalSizes(NS ns, int64_t out[4])
{
  if (!ns || !out) return E_ARG_NULL;
  if (!ns->setupcalled) return E_ARG_WRONGSTATE;
  FLABI(fl_poisson_sizes(ns->poisson, out));
  return 0;
}

FlErrorCode NSPressureCorrection(NS ns, double *vstar[3], double *Vstar[3], const double *contrhs, double *dp, fl_ksp_stats *stats)
{
  if (!ns || !Vstar || !dp) return E_ARG_NULL;
  if (!ns->setupcalled) return E_ARG_WRONGSTATE;
  fl_ksp_stats local;
  int64_t      sz[4];
  void        *srhs = NULL;
  FLABI(fl_poisson_sizes(ns->poisson, sz));
  FLABI(fl_malloc(ns->device, sizeof(double) * (size_t)sz[0], &srhs));       /* abf->Srhs, abfpc.c:68 */
  int rc = fl_poisson_rhs(ns->poisson, Vstar[0], Vstar[1], Vstar[2], contrhs, (double *)srhs); /* abfpc.c:75-76 */
  if (!rc) rc = fl_poisson_solve(ns->poisson, (const double *)srhs, dp, &ns->schur, stats ? stats : &local); /* abfpc.c:77 */
  if (!rc) rc = fl_poisson_project(ns->poisson, dp, vstar ? vstar[0] : NULL, vstar ? vstar[1] : NULL, vstar ? vstar[2] : NULL, Vstar[0], Vstar[1], Vstar[2]); /* abfpc.c:80-101 */
  if (!rc) rc = fl_poisson_synchronize(ns->poisson);
  fl_free(ns->device, srhs);
  return rc ? -rc : 0;
}

/* Immersed boundary by explicit direct forcing (build-defined: the reference only promises IBM, THEORY_GUIDE.md:130-132):
 * every step adds  spread(U_target - interp(v0))  to momrhs, i.e. the force density (U_target - U)/dt that would bring the
 * interpolated marker velocity to its target within the step, times dt.  Markers / volumes / targets are device arrays
 * owned by the caller; Utarget_dev may be NULL (body at rest). */
static void ibm_free_own(NS ns)
{
  for (int q = 0; q < 6; ++q) {
    if (ns->ibm_own[q]) fl_free(ns->device, ns->ibm_own[q]);
    ns->ibm_own[q] = NULL;
  }
  /* ... and what a moving body added */
  if (ns->ibm_ref) fl_free(ns->device, ns->ibm_ref);
  if (ns->ibm_mv) fl_free(ns->device, ns->ibm_mv);
  ns->ibm_ref = ns->ibm_mv = NULL;
  ns->ibm_cap = ns->ibm_Ucap = 0;
  ns->ibm_motion     = NULL;
  ns->ibm_motion_ctx = NULL;
  ns->ibm_X[0] = ns->ibm_X[1] = ns->ibm_X[2] = NULL;
  /* ... and the bodies; no force until the next step */
  if (ns->ibm_body_own) fl_free(ns->device, ns->ibm_body_own);
  ns->ibm_body_own = NULL;
  ns->ibm_body     = NULL;
  ns->ibm_nbody    = 0;
  ns->ibm_body_cap = 0;
  ns->ibm_force_ready = ns->ibm_have_centre = ns->ibm_have_centre0 = 0;
  ns->ibm_mon_step    = -1;
}

/* -ns_ibm_marker_distribution owner: this rank's share of the replicated arrays, gathered into arrays the NS owns -- ibm_own[0..2] positions, [3] volumes,
 * [4] targets (3 x Lloc, or NULL), [5] the global marker numbers.  Set-up time: through the host. */
static FlErrorCode ibm_gather_own(NS ns, int kind, int64_t L, const double *const src[5], int64_t *Lloc)
{
  void    *idx_dev = NULL;
  int64_t  n = 0, *idx = NULL;
  double  *in = NULL, *out = NULL;
  int      rc = fl_malloc(ns->device, sizeof(int64_t) * (size_t)L, &idx_dev);
  if (!rc) rc = fl_ibm_owned_select(ns->poisson, kind, L, src[0], src[1], src[2], (int64_t *)idx_dev, &n);
  if (!rc) {
    idx = (int64_t *)malloc(sizeof(int64_t) * (size_t)(n + 1));
    in  = (double *)malloc(sizeof(double) * 3 * (size_t)L);
    out = (double *)malloc(sizeof(double) * 3 * (size_t)(n + 1));
    if (!idx || !in || !out) rc = -E_MEM;
  }
  if (!rc && n > 0) rc = fl_memcpy_d2h(ns->device, idx, idx_dev, sizeof(int64_t) * (size_t)n);
  for (int q = 0; q < 5 && !rc; ++q) {
    if (!src[q]) continue;
    const int ncomp = q == 4 ? 3 : 1;
    rc = fl_memcpy_d2h(ns->device, in, src[q], sizeof(double) * (size_t)(ncomp * L));
    for (int c = 0; c < ncomp; ++c)
      for (int64_t a = 0; a < n; ++a) out[c * n + a] = in[c * L + idx[a]];
    if (!rc) rc = fl_malloc(ns->device, sizeof(double) * (size_t)(ncomp * n + 1), &ns->ibm_own[q]);
    if (!rc && n > 0) rc = fl_memcpy_h2d(ns->device, ns->ibm_own[q], out, sizeof(double) * (size_t)(ncomp * n));
  }
  if (!rc) rc = fl_malloc(ns->device, sizeof(int64_t) * (size_t)(n + 1), &ns->ibm_own[5]);
  if (!rc && n > 0) rc = fl_memcpy_h2d(ns->device, ns->ibm_own[5], idx, sizeof(int64_t) * (size_t)n);
  free(idx);
  free(in);
  free(out);
  if (idx_dev) fl_free(ns->device, idx_dev);
  *Lloc = n;
  return rc ? -rc : 0;
}

FlErrorCode NSSetImmersedBoundary(NS ns, int kind, int64_t L, const double *X_dev, const double *Y_dev, const double *Z_dev, const double *dV_dev, const double *Utarget_dev)
{
  if (!ns || !X_dev || !Y_dev || !Z_dev || !dV_dev) return E_ARG_NULL;
  if (!ns->setupcalled) return E_ARG_WRONGSTATE;
  if (L < 1) return E_ARG_OUTOFRANGE;
  scalars_ibm_off(ns);
  if (ns->ibm) {
    fl_ibm_destroy(ns->ibm);
    ns->ibm = NULL;
  }
  if (ns->ibm_U) fl_free(ns->device, ns->ibm_U);
  ns->ibm_U = NULL;
  ibm_free_own(ns);
  void *u = NULL;
  ns->ibm_Lglobal = L;
  if (ns->ibm_owner) {
    /* the caller still hands over the replicated arrays; every rank keeps what the ownership rule gives it (the global index is the marker number,
     * so the forcing adds up in the replicated order) */
    const double *const src[5] = {X_dev, Y_dev, Z_dev, dV_dev, Utarget_dev};
    int64_t             Lloc   = 0;
    FLCHK(ibm_gather_own(ns, kind, L, src, &Lloc));
    FLABI(fl_ibm_create_owned(ns->poisson, kind, Lloc, (const double *)ns->ibm_own[0], (const double *)ns->ibm_own[1], (const double *)ns->ibm_own[2], (const int64_t *)ns->ibm_own[5], &ns->ibm));
    FLABI(fl_malloc(ns->device, sizeof(double) * (3 * (size_t)Lloc + 1), &u));
    ns->ibm_U  = (double *)u;
    ns->ibm_L  = Lloc;
    ns->ibm_dV = (const double *)ns->ibm_own[3];
    ns->ibm_Ut = (const double *)ns->ibm_own[4];
    for (int d = 0; d < 3; ++d) ns->ibm_X[d] = (const double *)ns->ibm_own[d];
    ns->ibm_Ucap = Lloc;
    return 0;
  }
  FLABI(fl_ibm_create(ns->poisson, kind, L, X_dev, Y_dev, Z_dev, &ns->ibm));
  FLABI(fl_malloc(ns->device, sizeof(double) * 3 * (size_t)L, &u));
  ns->ibm_U  = (double *)u;
  ns->ibm_L  = L;
  ns->ibm_dV = dV_dev;
  ns->ibm_Ut = Utarget_dev;
  ns->ibm_X[0] = X_dev, ns->ibm_X[1] = Y_dev, ns->ibm_X[2] = Z_dev;
  ns->ibm_Ucap = L;
  return 0;
}

/* room for n markers in ibm_ref (5 n: the fifth row carries the body ids of NSSetImmersedBoundaryBodies) and ibm_mv (6 n); the old contents are not kept */
static FlErrorCode ibm_motion_reserve(NS ns, int64_t n)
{
  if (ns->ibm_ref && ns->ibm_mv && n <= ns->ibm_cap) return 0;
  if (ns->ibm_ref) fl_free(ns->device, ns->ibm_ref);
  if (ns->ibm_mv) fl_free(ns->device, ns->ibm_mv);
  ns->ibm_ref = ns->ibm_mv = NULL;
  ns->ibm_cap = 0;
  const int64_t cap = n + n / 4 + 64;
  void         *a = NULL, *b = NULL;
  FLABI(fl_malloc(ns->device, sizeof(double) * 5 * (size_t)cap, &a));
  ns->ibm_ref = (double *)a;
  FLABI(fl_malloc(ns->device, sizeof(double) * 6 * (size_t)cap, &b));
  ns->ibm_mv  = (double *)b;
  ns->ibm_cap = cap;
  return 0;
}

FlErrorCode NSSetImmersedBoundaryMotion(NS ns, const double centre0[3], NSBodyMotionFn fn, void *ctx)
{
  if (!ns) return E_ARG_NULL;
  if (!ns->setupcalled || !ns->ibm) return E_ARG_WRONGSTATE;
  if (!fn) { /* at rest where it is: the set keeps the last positions, the target is zero */
    if (ns->ibm_motion) ns->ibm_Ut = NULL;
    ns->ibm_motion     = NULL;
    ns->ibm_motion_ctx = NULL;
    if (centre0 && !ns->ibm_have_centre) { /* a body that never moved: the point NSGetImmersedBoundaryForce refers its torque to */
      for (int d = 0; d < 3; ++d) ns->ibm_centre0[d] = centre0[d];
      ns->ibm_have_centre0 = 1;
    }
    return 0;
  }
  if (!centre0) return E_ARG_NULL;
  if (!ns->ibm_ref) {
    /* the reference pose: the markers as NSSetImmersedBoundary received them, and their volumes, in arrays that follow the markers from now on */
    const int64_t L = ns->ibm_L;
    FLCHK(ibm_motion_reserve(ns, L));
    if (L > 0) {
      for (int d = 0; d < 3; ++d) FLABI(fl_vec_lincomb(ns->poisson, L, 1., ns->ibm_X[d], 0., NULL, ns->ibm_ref + d * L));
      FLABI(fl_vec_lincomb(ns->poisson, L, 1., ns->ibm_dV, 0., NULL, ns->ibm_ref + 3 * L));
    }
    ns->ibm_dV = ns->ibm_ref + 3 * L;
    if (ns->ibm_owner) { /* the copies made at NSSetImmersedBoundary are in an order the first migration ends */
      FLABI(fl_poisson_synchronize(ns->poisson));
      for (int q = 0; q < 5; ++q) {
        if (ns->ibm_own[q]) fl_free(ns->device, ns->ibm_own[q]);
        ns->ibm_own[q] = NULL;
      }
      ns->ibm_X[0] = ns->ibm_X[1] = ns->ibm_X[2] = NULL;
    }
  }
  for (int d = 0; d < 3; ++d) ns->ibm_centre0[d] = centre0[d];
  ns->ibm_have_centre0 = 1;
  ns->ibm_motion     = fn;
  ns->ibm_motion_ctx = ctx;
  return ibm_body_to_ref(ns);
}

/* the moving body at t + dt: pose from the callback, markers moved (and, owner-rank markers, handed from rank to rank), target velocities */
static FlErrorCode ibm_move(NS ns)
{
  double centre[3] = {0., 0., 0.}, rotvec[3] = {0., 0., 0.}, vel[3] = {0., 0., 0.}, omega[3] = {0., 0., 0.};
  FlErrorCode rc = ns->ibm_motion(ns->t + ns->dt, centre, rotvec, vel, omega, ns->ibm_motion_ctx);
  if (ns->mesh->size > 1) { /* every rank leaves the step together */
    double v[2] = {rc ? 1. : 0., (double)rc};
    FLABI(fl_poisson_allreduce_sum(ns->poisson, v, 2));
    if (!rc && v[0] > 0.) rc = (FlErrorCode)(v[1] / v[0] + (v[1] >= 0. ? 0.5 : -0.5));
  }
  if (rc) return rc;
  for (int d = 0; d < 3; ++d) ns->ibm_centre[d] = centre[d];
  ns->ibm_have_centre = 1;
  fl_poisson *h = ns->poisson;
  int64_t     L = ns->ibm_L;
  double     *ref = ns->ibm_ref, *pos = ns->ibm_mv;
  if (!ns->ibm_owner) {
    double *Ut = ns->ibm_mv + 3 * ns->ibm_cap;
    FLABI(fl_ibm_rigid_pose(h, L, ref, ref + L, ref + 2 * L, ns->ibm_centre0, centre, rotvec, vel, omega, pos, pos + L, pos + 2 * L, Ut));
    FLABI(fl_ibm_update(ns->ibm, pos, pos + L, pos + 2 * L));
    ns->ibm_Ut = Ut;
    return 0;
  }
  int64_t Ln = 0, moved[2] = {0, 0};
  FLABI(fl_ibm_rigid_pose(h, L, ref, ref + L, ref + 2 * L, ns->ibm_centre0, centre, rotvec, vel, omega, pos, pos + L, pos + 2 * L, NULL));
  const int nattr = ns->ibm_body_own ? 5 : 4; /* reference position, volume and, with several bodies, the body id */
  FLABI(fl_ibm_migrate(ns->ibm, L ? pos : NULL, L ? pos + L : NULL, L ? pos + 2 * L : NULL, nattr, L ? ref : NULL, &Ln, moved));
  /* the set holds positions, numbers and the four attributes now: the NS's arrays follow the new count */
  FLCHK(ibm_motion_reserve(ns, Ln));
  ref = ns->ibm_ref;
  pos = ns->ibm_mv;
  FLABI(fl_ibm_owned_fetch(ns->ibm, ns->ibm_cap, NULL, NULL, NULL, NULL, nattr, ref));
  if (nattr == 5 && (moved[0] > 0 || moved[1] > 0)) FLCHK(ibm_body_from_ref(ns, Ln)); /* the list of this rank has changed: its ids follow */
  if (Ln > ns->ibm_Ucap) {
    void *u = NULL;
    FLABI(fl_poisson_synchronize(h));
    if (ns->ibm_U) fl_free(ns->device, ns->ibm_U);
    ns->ibm_U = NULL;
    FLABI(fl_malloc(ns->device, sizeof(double) * 3 * (size_t)ns->ibm_cap, &u));
    ns->ibm_U    = (double *)u;
    ns->ibm_Ucap = ns->ibm_cap;
  }
  double *Ut = ns->ibm_mv + 3 * ns->ibm_cap;
  FLABI(fl_ibm_rigid_pose(h, Ln, ref, ref + Ln, ref + 2 * Ln, ns->ibm_centre0, centre, rotvec, vel, omega, NULL, NULL, NULL, Ut));
  ns->ibm_L  = Ln;
  ns->ibm_dV = ref + 3 * Ln;
  ns->ibm_Ut = Ut;
  return 0;
}

FlErrorCode NSGetImmersedBoundary(NS ns, fl_ibm **ibm)
{
  if (!ns || !ibm) return E_ARG_NULL;
  if (!ns->ibm) return E_ARG_WRONGSTATE;
  *ibm = ns->ibm;
  return 0;
}


/* ---- force and torque on the bodies -------------------------------------------------------------------------------------------------- */

/* owner distribution under a prescribed motion: the ids as the fifth row of ibm_ref (doubles), so that they travel through fl_ibm_migrate */
static FlErrorCode ibm_body_to_ref(NS ns)
{
  const int64_t L = ns->ibm_L;
  if (!ns->ibm_owner || !ns->ibm_ref || !ns->ibm_body_own || L == 0) return 0;
  int32_t *ids = (int32_t *)malloc(sizeof(int32_t) * (size_t)L);
  double  *val = (double *)malloc(sizeof(double) * (size_t)L);
  int      rc  = (!ids || !val) ? -E_MEM : 0;
  if (!rc) rc = fl_poisson_synchronize(ns->poisson);
  if (!rc) rc = fl_memcpy_d2h(ns->device, ids, ns->ibm_body_own, sizeof(int32_t) * (size_t)L);
  for (int64_t l = 0; l < L && !rc; ++l) val[l] = (double)ids[l];
  if (!rc) rc = fl_memcpy_h2d(ns->device, ns->ibm_ref + 4 * L, val, sizeof(double) * (size_t)L);
  free(ids);
  free(val);
  return rc ? -rc : 0;
}
/* ... and back after a migration: ibm_body_own from the fifth row of ibm_ref (Ln markers) */
static FlErrorCode ibm_body_from_ref(NS ns, int64_t Ln)
{
  if (Ln > ns->ibm_body_cap) {
    void *b = NULL;
    FLABI(fl_poisson_synchronize(ns->poisson));
    if (ns->ibm_body_own) fl_free(ns->device, ns->ibm_body_own);
    ns->ibm_body_own = NULL;
    ns->ibm_body     = NULL;
    ns->ibm_body_cap = 0;
    FLABI(fl_malloc(ns->device, sizeof(int32_t) * (size_t)(ns->ibm_cap + 1), &b));
    ns->ibm_body_own = b;
    ns->ibm_body_cap = ns->ibm_cap;
  }
  ns->ibm_body = (const int32_t *)ns->ibm_body_own;
  if (Ln == 0) return 0;
  int32_t *ids = (int32_t *)malloc(sizeof(int32_t) * (size_t)Ln);
  double  *val = (double *)malloc(sizeof(double) * (size_t)Ln);
  int      rc  = (!ids || !val) ? -E_MEM : 0;
  if (!rc) rc = fl_poisson_synchronize(ns->poisson);
  if (!rc) rc = fl_memcpy_d2h(ns->device, val, ns->ibm_ref + 4 * Ln, sizeof(double) * (size_t)Ln);
  for (int64_t l = 0; l < Ln && !rc; ++l) ids[l] = (int32_t)val[l];
  if (!rc) rc = fl_memcpy_h2d(ns->device, ns->ibm_body_own, ids, sizeof(int32_t) * (size_t)Ln);
  free(ids);
  free(val);
  return rc ? -rc : 0;
}

FlErrorCode NSSetImmersedBoundaryBodies(NS ns, int nbody, const int32_t *body_dev)
{
  if (!ns) return E_ARG_NULL;
  if (nbody < 1 || nbody > 64) return E_ARG_OUTOFRANGE;
  if (!ns->setupcalled || !ns->ibm) return E_ARG_WRONGSTATE;
  if (!body_dev) return E_ARG_NULL;
  scalars_ibm_off(ns);
  if (!ns->ibm_owner) {
    ns->ibm_nbody = nbody;
    ns->ibm_body  = body_dev;
    return 0;
  }
  /* this rank's share: the set knows the numbers (= indices into the list) of the markers it owns now, before or after any migration */
  const int64_t n = ns->ibm_L, L = ns->ibm_Lglobal;
  void         *gid_dev = NULL, *own = NULL;
  int64_t      *gid = (int64_t *)malloc(sizeof(int64_t) * (size_t)(n + 1));
  int32_t      *all = (int32_t *)malloc(sizeof(int32_t) * (size_t)L), *mine = (int32_t *)malloc(sizeof(int32_t) * (size_t)(n + 1));
  int           rc  = (!gid || !all || !mine) ? -E_MEM : 0;
  const int64_t cap = ns->ibm_cap > n ? ns->ibm_cap : n;
  if (!rc) rc = fl_malloc(ns->device, sizeof(int64_t) * (size_t)(n + 1), &gid_dev);
  if (!rc) rc = fl_ibm_owned_fetch(ns->ibm, n, NULL, NULL, NULL, (int64_t *)gid_dev, 0, NULL);
  if (!rc) rc = fl_poisson_synchronize(ns->poisson);
  if (!rc && n > 0) rc = fl_memcpy_d2h(ns->device, gid, gid_dev, sizeof(int64_t) * (size_t)n);
  if (!rc) rc = fl_memcpy_d2h(ns->device, all, body_dev, sizeof(int32_t) * (size_t)L);
  for (int64_t a = 0; a < n && !rc; ++a) {
    if (gid[a] < 0 || gid[a] >= L) rc = -E_ARG_OUTOFRANGE;
    else mine[a] = all[gid[a]];
  }
  if (!rc) rc = fl_malloc(ns->device, sizeof(int32_t) * (size_t)(cap + 1), &own);
  if (!rc && n > 0) rc = fl_memcpy_h2d(ns->device, own, mine, sizeof(int32_t) * (size_t)n);
  free(gid);
  free(all);
  free(mine);
  if (gid_dev) fl_free(ns->device, gid_dev);
  if (rc) {
    if (own) fl_free(ns->device, own);
    return -rc;
  }
  if (ns->ibm_body_own) fl_free(ns->device, ns->ibm_body_own);
  ns->ibm_body_own = own;
  ns->ibm_body_cap = cap;
  ns->ibm_body     = (const int32_t *)own;
  ns->ibm_nbody    = nbody;
  return ibm_body_to_ref(ns);
}

/* about == NULL: the point every body's torque refers to */
static void ibm_default_about(NS ns, double p[3])
{
  for (int d = 0; d < 3; ++d) p[d] = ns->ibm_have_centre ? ns->ibm_centre[d] : (ns->ibm_have_centre0 ? ns->ibm_centre0[d] : 0.);
}

FlErrorCode NSGetImmersedBoundaryForce(NS ns, const double *about, double *force, double *torque)
{
  if (!ns || !force) return E_ARG_NULL;
  if (!ns->ibm || !ns->ibm_force_ready) return E_ARG_WRONGSTATE;
  const int     nbody = ns->ibm_nbody ? ns->ibm_nbody : 1;
  const int64_t L     = ns->ibm_L;
  double        ab[3 * 64], f[3 * 64], t[3 * 64];
  for (int b = 0; b < nbody; ++b) {
    if (about) memcpy(ab + 3 * b, about + 3 * b, sizeof(double) * 3);
    else ibm_default_about(ns, ab + 3 * b);
  }
  FLABI(fl_ibm_force(ns->ibm, L > 0 ? ns->ibm_U : NULL, L > 0 ? ns->ibm_dV : NULL, ns->ibm_nbody ? ns->ibm_body : NULL, nbody, ab, f, torque ? t : NULL));
  const double s = -(ns->rho / ns->dt); /* the fluid's reaction to the forcing density (U_target - U) rho / dt */
  for (int a = 0; a < 3 * nbody; ++a) {
    force[a] = s * f[a];
    if (torque) torque[a] = s * t[a];
  }
  return 0;
}

FlErrorCode NSMonitorImmersedBoundaryForce(NS ns, void *ctx)
{
  if (!ns || !ctx) return E_ARG_NULL;
  if (!ns->ibm || !ns->ibm_force_ready || ns->ibm_mon_step == ns->step) return 0;
  const int nbody = ns->ibm_nbody ? ns->ibm_nbody : 1;
  double    f[3 * 64], t[3 * 64];
  FLCHK(NSGetImmersedBoundaryForce(ns, NULL, f, t));
  ns->ibm_mon_step = ns->step;
  if (ns->mesh && ns->mesh->rank != 0) return 0;
  FILE *fp = fopen((const char *)ctx, "a");
  if (!fp) return E_FILE_OPEN;
  int bad = 0;
  for (int b = 0; b < nbody; ++b)
    bad |= fprintf(fp, "%lld %.17g %d %.17g %.17g %.17g %.17g %.17g %.17g\n", (long long)ns->step, ns->t, b, f[3 * b], f[3 * b + 1], f[3 * b + 2], t[3 * b], t[3 * b + 1], t[3 * b + 2]) < 0;
  bad |= fclose(fp) != 0;
  return bad ? E_FILE_WRITE : 0;
}
static FlErrorCode ibm_force_monitor_destroy(void **ctx)
{
  free(*ctx);
  *ctx = NULL;
  return 0;
}

FlErrorCode NSGetMomentumKSPOptions(NS ns, fl_ksp_opts **opts)
{
  if (!ns || !opts) return E_ARG_NULL;
  *opts = &ns->mom;
  return 0;
}

/* The A block of NSFormJacobian (cnlinearcart3d.c:2930-2941): A = I + dt C(V0, v0interp) - (mu dt / 2 rho) L */
FlErrorCode NSSetPreviousState(NS ns, const double *const V0[3], const double *const v0interp[9])
{
  if (!ns || !V0 || !v0interp) return E_ARG_NULL;
  if (!ns->setupcalled) return E_ARG_WRONGSTATE;
  FLCHK(ns_jacobian(ns));
  FLABI(fl_momentum_set_state(ns->momentum, ns->dt, ns->rho, ns->mu, V0, v0interp));
  return 0;
}

FlErrorCode NSGetMomentum(NS ns, fl_momentum **momentum)
{
  if (!ns || !momentum) return E_ARG_NULL;
  if (!ns->momentum) return E_ARG_WRONGSTATE;
  *momentum = ns->momentum;
  return 0;
}

/* PCApply_ABF, abfpc.c:48-111 */
FlErrorCode NSApplyPreconditioner(NS ns, const double *momrhs, const double *const interprhs[3], const double *contrhs, double *v, double *const V[3], double *p, fl_ksp_stats stats[2])
{
  if (!ns || !momrhs || !v || !V || !p) return E_ARG_NULL;
  if (!ns->setupcalled || !ns->momentum) return E_ARG_WRONGSTATE; /* "NSSetPreviousState first": A does not exist yet */
  fl_ksp_stats local[2];
  int          rc = fl_abf_apply(ns->momentum, &ns->mom, &ns->schur, momrhs, interprhs, contrhs, v, V, p, stats ? stats : local);
  if (!rc) rc = fl_poisson_synchronize(ns->poisson);
  return rc ? -rc : 0;
}

FlErrorCode NSUpdatePressure(NS ns, const double *dp, const double *p0, double *phalf, double *p)
{
  if (!ns) return E_ARG_NULL;
  if (!ns->setupcalled) return E_ARG_WRONGSTATE;
  FLABI(fl_pressure_update(ns->poisson, ns->step == 0, dp, p0, phalf, p)); /* cnlinearcart3d.c:2846-2854 */
  ++ns->step;                                                                /* nsbasic.c:288-291 */
  ns->t += ns->dt;
  return 0;
}

FlErrorCode NSComputeStaggeredPressureGradientBC(NS ns, double t, double *V[3])
{
  if (!ns || !V) return E_ARG_NULL;
  if (!ns->setupcalled) return E_ARG_WRONGSTATE;
  Mesh_Cart       *cart = (Mesh_Cart *)ns->mesh->data;
  const fl_decomp *D    = &ns->mesh->decomp;
  for (int b = 0; b < 6; ++b) {
    if (ns->bcs[b].type != NS_BC_PRESSURE_OUTLET) continue;
    const int ax = b / 2, side = b % 2;
    if (side ? (D->coord[ax] != D->ranks[ax] - 1) : (D->coord[ax] != 0)) continue; /* isFirstRank / isLastRank */
    if (!ns->bcs[b].pressure) return E_ARG_WRONGSTATE;
    const int     a1 = ax == 0 ? 1 : 0, a2 = ax == 2 ? 1 : 2; /* the two in-plane axes, a1 fastest */
    const int64_t n1 = D->len[a1], n2 = D->len[a2];
    double       *pb = (double *)malloc(sizeof(double) * (size_t)(n1 * n2));
    if (!pb) return E_MEM;
    for (int64_t j = 0; j < n2; ++j)
      for (int64_t i = 0; i < n1; ++i) {
        double xb[3], val = 0.;
        xb[ax] = cart->xf[ax][side ? cart->N[ax] : 0];
        xb[a1] = cart->xc[a1][D->lo[a1] + i];
        xb[a2] = cart->xc[a2][D->lo[a2] + j];
        FlErrorCode e = ns->bcs[b].pressure(3, t, xb, &val, ns->bcs[b].ctx_pressure);
        if (e) {
          free(pb);
          return e;
        }
        pb[j * n1 + i] = val;
      }
    void *pbd = NULL;
    int   rc  = fl_malloc(ns->device, sizeof(double) * (size_t)(n1 * n2), &pbd);
    if (!rc) rc = fl_memcpy_h2d(ns->device, pbd, pb, sizeof(double) * (size_t)(n1 * n2));
    if (!rc) rc = fl_poisson_gst_bc(ns->poisson, b, (const double *)pbd, V[ax]);
    if (!rc) rc = fl_poisson_synchronize(ns->poisson);
    fl_free(ns->device, pbd);
    free(pb);
    if (rc) return -rc;
  }
  return 0;
}

/* ---- NSCNLINEAR: the shipped type (fluca/src/ns/impl/linearcn/) ------------------------------------------------------
 * The fields and the step of NSStep_CNLinear_Cart3d_Internal / NSFormJacobian / NSFormFunction (cnlinearcart3d.c:2807-3060)
 * on device arrays, for all four boundary-condition types.  Outer solve:
 * -ns_ksp_type richardson (x += PCApply_ABF(f - J x), unpreconditioned norm, -ns_ksp_rtol) or preonly. */
static FlErrorCode cnl_alloc(NS ns, double **p, int64_t n)
{
  void *d = NULL;
  FLABI(fl_malloc(ns->device, sizeof(double) * (size_t)(n > 0 ? n : 1), &d));
  *p = (double *)d;
  return 0;
}

static FlErrorCode NSSetUp_CNLinear(NS ns)
{
  NS_CNLinear *c = (NS_CNLinear *)calloc(1, sizeof(*c));
  if (!c) return E_MEM;
  ns->data = c;
  FLABI(fl_poisson_sizes(ns->poisson, c->sz));
  const int64_t N = c->sz[0];
  double      **cellv[] = {&c->sol_v, &c->sol0_v, &c->x_v, &c->f_v, &c->r_v, &c->d_v};
  double      **cells[] = {&c->sol_p, &c->sol0_p, &c->phalf, &c->x_p, &c->f_p, &c->r_p, &c->d_p};
  for (size_t a = 0; a < sizeof(cellv) / sizeof(cellv[0]); ++a) FLCHK(cnl_alloc(ns, cellv[a], 3 * N));
  for (size_t a = 0; a < sizeof(cells) / sizeof(cells[0]); ++a) FLCHK(cnl_alloc(ns, cells[a], N));
  int64_t pmax = 1;
  for (int d = 0; d < 3; ++d) {
    double **faces[] = {&c->sol_V[d], &c->sol0_V[d], &c->x_V[d], &c->f_V[d], &c->r_V[d], &c->d_V[d]};
    for (size_t a = 0; a < sizeof(faces) / sizeof(faces[0]); ++a) FLCHK(cnl_alloc(ns, faces[a], c->sz[1 + d]));
    for (int q = 0; q < 3; ++q) FLCHK(cnl_alloc(ns, &c->W[q * 3 + d], c->sz[1 + d]));
    const int     a1 = d == 0 ? 1 : 0, a2 = d == 2 ? 1 : 2;
    const int64_t pl = ns->mesh->decomp.len[a1] * ns->mesh->decomp.len[a2];
    if (pl > pmax) pmax = pl;
  }
  c->plane_cap = pmax;
  FLCHK(cnl_alloc(ns, &c->plane_dev, pmax));
  for (int q = 0; q < 7; ++q) FLABI(fl_malloc_host(sizeof(double) * (size_t)pmax, (void **)&c->plane_host[q]));
  return 0;
}

static FlErrorCode NSDestroy_CNLinear(NS ns)
{
  NS_CNLinear *c = (NS_CNLinear *)ns->data;
  if (!c) return 0;
  double *cell[] = {c->sol_v, c->sol0_v, c->x_v, c->f_v, c->r_v, c->d_v, c->sol_p, c->sol0_p, c->phalf, c->x_p, c->f_p, c->r_p, c->d_p, c->plane_dev};
  for (size_t a = 0; a < sizeof(cell) / sizeof(cell[0]); ++a)
    if (cell[a]) fl_free(ns->device, cell[a]);
  for (int d = 0; d < 3; ++d) {
    double *f[] = {c->sol_V[d], c->sol0_V[d], c->x_V[d], c->f_V[d], c->r_V[d], c->d_V[d], c->W[d], c->W[3 + d], c->W[6 + d]};
    for (size_t a = 0; a < sizeof(f) / sizeof(f[0]); ++a)
      if (f[a]) fl_free(ns->device, f[a]);
  }
  for (int q = 0; q < 7; ++q) fl_free_host(c->plane_host[q]);
  for (int b = 0; b < 6; ++b)
    for (int k = 0; k < 2; ++k)
      for (int q = 0; q < 3; ++q) fl_free_host(c->bc_plane[b][k][q]);
  for (int i = -2; i < c->gm_cap; ++i) { /* every slot of the table: a failed allocation may have left a partly filled one */
    NSVec   *a = i == -2 ? &c->gm_w : i == -1 ? &c->gm_t : &c->gm_V[i];
    double *q[5] = {a->v, a->p, a->V[0], a->V[1], a->V[2]};
    for (int k = 0; k < 5; ++k)
      if (q[k]) fl_free(ns->device, q[k]);
  }
  free(c->gm_V);
  free(c);
  ns->data = NULL;
  return 0;
}

FlErrorCode NSGetPressureHalfStep(NS ns, double **phalf) /* cnl->phalf, "PressureHalfStep" (cnlinear.c:54) */
{
  if (!ns || !phalf) return E_ARG_NULL;
  if (!ns->setupcalled || !ns->data) return E_ARG_WRONGSTATE;
  *phalf = ((NS_CNLinear *)ns->data)->phalf;
  return 0;
}
FlErrorCode NSGetMesh(NS ns, Mesh *mesh)
{
  if (!ns || !mesh) return E_ARG_NULL;
  *mesh = ns->mesh;
  return 0;
}
FlErrorCode NSGetDevice(NS ns, int *device)
{
  if (!ns || !device) return E_ARG_NULL;
  *device = ns->device;
  return 0;
}
FlErrorCode NSSetTimeStepAndTime(NS ns, int64_t step, double t) /* what NSLoadSolution does last, nssol.c:199-201 */
{
  if (!ns) return E_ARG_NULL;
  if (step < 0) return E_ARG_OUTOFRANGE;
  ns->step = step;
  ns->t    = t;
  return 0;
}
FlErrorCode NSBarrier(NS ns) /* MPI_Barrier(PetscObjectComm(ns)) */
{
  if (!ns) return E_ARG_NULL;
  if (!ns->setupcalled) return E_ARG_WRONGSTATE;
  FLABI(fl_poisson_barrier(ns->poisson));
  return 0;
}
FlErrorCode NSGetSolutionArrays(NS ns, double **v, double *V[3], double **p)
{
  if (!ns) return E_ARG_NULL;
  if (!ns->setupcalled || !ns->data) return E_ARG_WRONGSTATE;
  NS_CNLinear *c = (NS_CNLinear *)ns->data;
  if (v) *v = c->sol_v;
  if (p) *p = c->sol_p;
  if (V)
    for (int d = 0; d < 3; ++d) V[d] = c->sol_V[d];
  return 0;
}

/* boundary b touches this rank and carries a velocity condition: the callback at the face centres, out[c] = component c on this rank's part of
 * the boundary (cnlinearcart3d.c:690-698: xb = face coordinate, cell centres in plane).  A step looks at the values at t and t + dt several times
 * (the boundary-condition vectors of L, C, B and the wall faces of v0interp), and its t + dt is the next step's t: the planes of the two most recent
 * times are kept (page-locked, so that they can be handed over as they are) -- a callback is a function of (t, x) by its contract, and a plane
 * is evaluated again when the callback, its context or the time differ. */
static FlErrorCode cnl_eval_velocity(NS ns, int b, double t, const double *out[3])
{
  NS_CNLinear     *c = (NS_CNLinear *)ns->data;
  Mesh_Cart       *cart = (Mesh_Cart *)ns->mesh->data;
  const fl_decomp *D    = &ns->mesh->decomp;
  const int        ax = b / 2, side = b % 2, a1 = ax == 0 ? 1 : 0, a2 = ax == 2 ? 1 : 2;
  const int64_t    n1 = D->len[a1], n2 = D->len[a2];
  if (!ns->bcs[b].velocity) return E_ARG_WRONGSTATE;
  for (int k = 0; k < 2; ++k)
    if (c->bc_have[b][k] && c->bc_time[b][k] == t && c->bc_fn[b][k] == ns->bcs[b].velocity && c->bc_ctx[b][k] == ns->bcs[b].ctx_velocity) {
      for (int q = 0; q < 3; ++q) out[q] = c->bc_plane[b][k][q];
      c->bc_old[b] = 1 - k;
      return 0;
    }
  const int k = c->bc_old[b]; /* the slot not asked for last */
  FLABI(fl_poisson_upload_fence(ns->poisson)); /* an upload out of that slot may still be under way */
  c->bc_have[b][k] = 0;
  for (int q = 0; q < 3; ++q)
    if (!c->bc_plane[b][k][q]) FLABI(fl_malloc_host(sizeof(double) * (size_t)c->plane_cap, (void **)&c->bc_plane[b][k][q]));
  double *p0 = c->bc_plane[b][k][0], *p1 = c->bc_plane[b][k][1], *p2 = c->bc_plane[b][k][2];
  for (int64_t j = 0; j < n2; ++j)
    for (int64_t i = 0; i < n1; ++i) {
      double xb[3], val[3] = {0., 0., 0.};
      xb[ax] = cart->xf[ax][side ? cart->N[ax] : 0];
      xb[a1] = cart->xc[a1][D->lo[a1] + i];
      xb[a2] = cart->xc[a2][D->lo[a2] + j];
      FLCHK(ns->bcs[b].velocity(3, t, xb, val, ns->bcs[b].ctx_velocity));
      p0[j * n1 + i] = val[0];
      p1[j * n1 + i] = val[1];
      p2[j * n1 + i] = val[2];
    }
  c->bc_have[b][k] = 1;
  c->bc_time[b][k] = t;
  c->bc_fn[b][k]   = ns->bcs[b].velocity;
  c->bc_ctx[b][k]  = ns->bcs[b].ctx_velocity;
  c->bc_old[b]     = 1 - k;
  for (int q = 0; q < 3; ++q) out[q] = c->bc_plane[b][k][q];
  return 0;
}

static int cnl_touches(NS ns, int b)
{
  const fl_decomp *D = &ns->mesh->decomp;
  return b % 2 ? D->coord[b / 2] == D->ranks[b / 2] - 1 : D->coord[b / 2] == 0;
}

/* host (page-locked: a scratch plane of cnl_scratch or a kept boundary plane) -> plane_dev, ordered on the handle's stream behind the kernel that read
 * the plane before and in front of the one that reads this one; the host plane stays untouched until the next fence */
static FlErrorCode cnl_upload(NS ns, const double *host, int64_t n)
{
  NS_CNLinear *c = (NS_CNLinear *)ns->data;
  FLABI(fl_poisson_upload(ns->poisson, c->plane_dev, host, sizeof(double) * (size_t)n));
  return 0;
}
/* the next of the seven page-locked scratch planes; once round, the uploads out of them are waited for */
static FlErrorCode cnl_scratch(NS ns, double **plane)
{
  NS_CNLinear *c = (NS_CNLinear *)ns->data;
  if (c->plane_next == 7) {
    FLABI(fl_poisson_upload_fence(ns->poisson));
    c->plane_next = 0;
  }
  *plane = c->plane_host[c->plane_next++];
  return 0;
}

/* r = f - J x  and its 2-norm over (v, V, p) */
static FlErrorCode cnl_residual(NS ns, double *rnorm)
{
  NS_CNLinear *c = (NS_CNLinear *)ns->data;
  fl_poisson  *h = ns->poisson;
  const double *xV[3] = {c->x_V[0], c->x_V[1], c->x_V[2]};
  FLABI(fl_abf_jacobian_mult(ns->momentum, c->x_v, xV, c->x_p, c->r_v, c->r_V, c->r_p));
  double s = 0., part;
  FLABI(fl_vec_lincomb(h, 3 * c->sz[0], -1., c->r_v, 1., c->f_v, c->r_v));
  FLABI(fl_vec_dot(h, 3 * c->sz[0], c->r_v, c->r_v, &part));
  s += part;
  for (int d = 0; d < 3; ++d) {
    FLABI(fl_vec_lincomb(h, c->sz[1 + d], -1., c->r_V[d], 1., c->f_V[d], c->r_V[d]));
    FLABI(fl_vec_dot(h, c->sz[1 + d], c->r_V[d], c->r_V[d], &part));
    s += part;
  }
  FLABI(fl_vec_lincomb(h, c->sz[0], -1., c->r_p, 1., c->f_p, c->r_p));
  FLABI(fl_vec_dot(h, c->sz[0], c->r_p, c->r_p, &part));
  s += part;
  *rnorm = sqrt(s);
  return 0;
}

/* ---- composite vectors (v: 3*cells, V[3]: faces, p: cells) for the outer Krylov method ------------------------------- */
static FlErrorCode cv_alloc(NS ns, NSVec *a)
{
  NS_CNLinear *c = (NS_CNLinear *)ns->data;
  FLCHK(cnl_alloc(ns, &a->v, 3 * c->sz[0]));
  FLCHK(cnl_alloc(ns, &a->p, c->sz[0]));
  for (int d = 0; d < 3; ++d) FLCHK(cnl_alloc(ns, &a->V[d], c->sz[1 + d]));
  return 0;
}
/* y = a x + b z (z may be NULL) */
static FlErrorCode cv_lincomb(NS ns, double a, const NSVec *x, double b, const NSVec *z, NSVec *y)
{
  NS_CNLinear *c = (NS_CNLinear *)ns->data;
  fl_poisson  *h = ns->poisson;
  FLABI(fl_vec_lincomb(h, 3 * c->sz[0], a, x->v, b, z ? z->v : NULL, y->v));
  FLABI(fl_vec_lincomb(h, c->sz[0], a, x->p, b, z ? z->p : NULL, y->p));
  for (int d = 0; d < 3; ++d) FLABI(fl_vec_lincomb(h, c->sz[1 + d], a, x->V[d], b, z ? z->V[d] : NULL, y->V[d]));
  return 0;
}
static FlErrorCode cv_dot(NS ns, const NSVec *x, const NSVec *y, double *out)
{
  NS_CNLinear *c = (NS_CNLinear *)ns->data;
  fl_poisson  *h = ns->poisson;
  double       s = 0., part;
  FLABI(fl_vec_dot(h, 3 * c->sz[0], x->v, y->v, &part));
  s += part;
  FLABI(fl_vec_dot(h, c->sz[0], x->p, y->p, &part));
  s += part;
  for (int d = 0; d < 3; ++d) {
    FLABI(fl_vec_dot(h, c->sz[1 + d], x->V[d], y->V[d], &part));
    s += part;
  }
  *out = s;
  return 0;
}
/* VecMDot / VecMAXPY on composite vectors: out[i] = x . Y[i] ; x -= sum_i coef[i] Y[i]   (k <= CV_MAXK) */
#define CV_MAXK 208
static FlErrorCode cv_mdot(NS ns, const NSVec *x, const NSVec *Y, int k, double *out)
{
  NS_CNLinear  *c = (NS_CNLinear *)ns->data;
  fl_poisson   *h = ns->poisson;
  const double *ys[CV_MAXK];
  double        part[CV_MAXK];
  if (k > CV_MAXK) return E_ARG_OUTOFRANGE;
  for (int i = 0; i < k; ++i) out[i] = 0.;
  for (int a = 0; a < 5; ++a) { /* v, p, V[0..2] */
    const int64_t n  = a == 0 ? 3 * c->sz[0] : a == 1 ? c->sz[0] : c->sz[a - 1];
    const double *xa = a == 0 ? x->v : a == 1 ? x->p : x->V[a - 2];
    for (int i = 0; i < k; ++i) ys[i] = a == 0 ? Y[i].v : a == 1 ? Y[i].p : Y[i].V[a - 2];
    FLABI(fl_vec_mdot(h, n, xa, ys, k, part));
    for (int i = 0; i < k; ++i) out[i] += part[i];
  }
  return 0;
}
static FlErrorCode cv_msub(NS ns, NSVec *x, const double *coef, const NSVec *Y, int k)
{
  NS_CNLinear  *c = (NS_CNLinear *)ns->data;
  fl_poisson   *h = ns->poisson;
  const double *ys[CV_MAXK];
  double        neg[CV_MAXK];
  if (k > CV_MAXK) return E_ARG_OUTOFRANGE;
  for (int i = 0; i < k; ++i) neg[i] = -coef[i];
  for (int a = 0; a < 5; ++a) {
    const int64_t n  = a == 0 ? 3 * c->sz[0] : a == 1 ? c->sz[0] : c->sz[a - 1];
    double       *xa = a == 0 ? x->v : a == 1 ? x->p : x->V[a - 2];
    for (int i = 0; i < k; ++i) ys[i] = a == 0 ? Y[i].v : a == 1 ? Y[i].p : Y[i].V[a - 2];
    FLABI(fl_vec_maxpy(h, n, xa, neg, ys, k));
  }
  return 0;
}
static FlErrorCode cv_pcapply(NS ns, const NSVec *r, NSVec *z) /* z = PCApply_ABF(r) */
{
  fl_ksp_stats  st[2];
  const double *rV[3] = {r->V[0], r->V[1], r->V[2]};
  FLABI(fl_abf_apply(ns->momentum, &ns->mom, &ns->schur, r->v, rV, r->p, z->v, z->V, z->p, st));
  ns->mom_its += st[0].iters;
  ns->schur_its += st[1].iters;
  if (st[0].reason == FL_DIVERGED_NANORINF || st[1].reason == FL_DIVERGED_NANORINF) ns->reason = -1;
  return 0;
}
static FlErrorCode cv_jmult(NS ns, const NSVec *x, NSVec *y) /* y = J x */
{
  const double *xV[3] = {x->V[0], x->V[1], x->V[2]};
  FLABI(fl_abf_jacobian_mult(ns->momentum, x->v, xV, x->p, y->v, y->V, y->p));
  return 0;
}

/* KSPGMRES as the reference's ns->snes uses it (nssol.c:21-29: rtol 1e-5, unpreconditioned norm => right preconditioning,
 * PETSc defaults: restart 30, classical Gram-Schmidt without refinement -- the same here).  Zero initial guess.  x = P^-1 (V y) at every restart / at the end.  PARITY UNPINNED like the
 * inner solvers (PETSc absent): restated from the published algorithm. */
static FlErrorCode cnl_gmres(NS ns, const NSVec *f, NSVec *x)
{
  const int    m = ns->gmres_restart;
  NS_CNLinear *c = (NS_CNLinear *)ns->data;
  if (c->gm_cap < m + 1) { /* the restart length grew: the basis table follows (the vectors in it stay) */
    NSVec *nv = (NSVec *)calloc((size_t)m + 1, sizeof(NSVec));
    if (!nv) return E_MEM;
    if (c->gm_V) memcpy(nv, c->gm_V, sizeof(NSVec) * (size_t)c->gm_nalloc);
    free(c->gm_V);
    c->gm_V   = nv;
    c->gm_cap = m + 1;
  }
  NSVec     *Vk = c->gm_V;
  NSVec     *w = &c->gm_w, *t = &c->gm_t; /* persistent work vectors */
  double   *H = (double *)calloc((size_t)(m + 1) * m, sizeof(double)), *cs = (double *)calloc(m, sizeof(double)), *sn = (double *)calloc(m, sizeof(double)),
           *g = (double *)calloc((size_t)m + 1, sizeof(double)), *y = (double *)calloc(m, sizeof(double));
  FlErrorCode rc = 0;
#define GM(call)          \
  do {                    \
    rc = (call);          \
    if (rc) goto done;    \
  } while (0)
  if (!H || !cs || !sn || !g || !y) {
    rc = E_MEM;
    goto done;
  }
  if (!w->v) GM(cv_alloc(ns, w));
  if (!t->v) GM(cv_alloc(ns, t));
  double fnorm, beta;
  GM(cv_dot(ns, f, f, &fnorm));
  fnorm = sqrt(fnorm);
  const double ttol = ns->ksp_rtol * fnorm > ns->ksp_atol ? ns->ksp_rtol * fnorm : ns->ksp_atol;
  GM(cv_lincomb(ns, 0., f, 0., NULL, x)); /* x = 0 */
  ns->ksp_its    = 0;
  ns->ksp_rnorm  = fnorm;
  ns->ksp_rnorm0 = fnorm;
  int first = 1;
  while (ns->reason >= 0) {
    /* r = f - J x */
    if (first) GM(cv_lincomb(ns, 1., f, 0., NULL, w));
    else {
      GM(cv_jmult(ns, x, w));
      GM(cv_lincomb(ns, -1., w, 1., f, w));
    }
    first = 0;
    GM(cv_dot(ns, w, w, &beta));
    beta          = sqrt(beta);
    ns->ksp_rnorm = beta;
    if (!(beta == beta)) { ns->reason = -1; break; }
    if (beta <= ttol || ns->ksp_its >= ns->ksp_max_it) break;
    if (c->gm_nalloc < 1) { GM(cv_alloc(ns, &Vk[0])); c->gm_nalloc = 1; }
    GM(cv_lincomb(ns, 1. / beta, w, 0., NULL, &Vk[0]));
    memset(g, 0, sizeof(double) * ((size_t)m + 1));
    g[0] = beta;
    int j = 0, conv = 0;
    for (; j < m && ns->ksp_its < ns->ksp_max_it; ++j) {
      GM(cv_pcapply(ns, &Vk[j], t)); /* z = P^-1 v_j */
      if (ns->reason < 0) break;
      GM(cv_jmult(ns, t, w));       /* w = J z */
      { /* classical Gram-Schmidt, no refinement (KSPGMRESClassicalGramSchmidtOrthogonalization, PETSc's default): all the
         * inner products from the same w in one pass (VecMDot), then one update (VecMAXPY) */
        double hcol[CV_MAXK];
        GM(cv_mdot(ns, w, Vk, j + 1, hcol));
        for (int i = 0; i <= j; ++i) H[i * m + j] = hcol[i];
        GM(cv_msub(ns, w, hcol, Vk, j + 1));
      }
      double hn;
      GM(cv_dot(ns, w, w, &hn));
      hn = sqrt(hn);
      H[(j + 1) * m + j] = hn;
      for (int i = 0; i < j; ++i) { /* previous Givens rotations on the new column */
        const double a = H[i * m + j], b = H[(i + 1) * m + j];
        H[i * m + j]       = cs[i] * a + sn[i] * b;
        H[(i + 1) * m + j] = -sn[i] * a + cs[i] * b;
      }
      {
        const double a = H[j * m + j], b = H[(j + 1) * m + j], r = hypot(a, b);
        cs[j] = r > 0. ? a / r : 1.;
        sn[j] = r > 0. ? b / r : 0.;
        H[j * m + j]       = r;
        H[(j + 1) * m + j] = 0.;
        g[j + 1]           = -sn[j] * g[j];
        g[j]               = cs[j] * g[j];
      }
      ++ns->ksp_its;
      ns->ksp_rnorm = fabs(g[j + 1]);
      if (ns->ksp_rnorm <= ttol || hn == 0.) {
        conv = 1;
        ++j;
        break;
      }
      if (j + 1 < m || 1) {
        if (c->gm_nalloc < j + 2) { GM(cv_alloc(ns, &Vk[j + 1])); c->gm_nalloc = j + 2; }
        GM(cv_lincomb(ns, 1. / hn, w, 0., NULL, &Vk[j + 1]));
      }
    }
    /* y = H^-1 g (back substitution), x += P^-1 (V y) */
    for (int i = j - 1; i >= 0; --i) {
      double sacc = g[i];
      for (int k = i + 1; k < j; ++k) sacc -= H[i * m + k] * y[k];
      y[i] = sacc / H[i * m + i];
    }
    if (j > 0) {
      GM(cv_lincomb(ns, y[0], &Vk[0], 0., NULL, w));
      for (int i = 1; i < j; ++i) GM(cv_lincomb(ns, 1., w, y[i], &Vk[i], w));
      GM(cv_pcapply(ns, w, t));
      GM(cv_lincomb(ns, 1., x, 1., t, x));
    }
    if (conv || ns->reason < 0) break;
  }
  if (ns->reason >= 0 && ns->ksp_rnorm > ttol && ns->ksp_its >= ns->ksp_max_it) ns->reason = -1;
done:
#undef GM
  free(H); free(cs); free(sn); free(g); free(y);
  return rc;
}

/* NSFormFunction_CNLinear (cnlinear.c:86-109 -> cnlinearcart3d.c:2945-3060): the right-hand side of the step.  x is not read
 * (the step is linear: SNESSetPicard, nsbasic.c:248).  Scratch: cnl->d_v, the host planes. */
static FlErrorCode NSFormFunction_CNLinear(NS ns, const NSVec *x, NSVec *f)
{
  NS_CNLinear *c = (NS_CNLinear *)ns->data;
  (void)x;
  if (!c || !f || !f->v || !f->p) return E_ARG_NULL;
  if (!c->have_sol0 || !ns->momentum) return E_ARG_WRONGSTATE; /* ns->sol0 is what the function is formed from */
  Mesh_Cart    *cart = (Mesh_Cart *)ns->mesh->data;
  fl_poisson   *h = ns->poisson;
  const int64_t N = c->sz[0];
  const double  dt = ns->dt, t = ns->t, cv = 0.5 * ns->mu * dt / ns->rho;
  /* momrhs = v0 + cv L v0 - kappa G p, :2976-2993 (p0 on the first step, phalf afterwards) */
  FLABI(fl_momentum_rhs(ns->momentum, dt, ns->rho, ns->mu, c->sol0_v, ns->step == 0 ? c->sol0_p : c->phalf, NULL, f->v));
  for (int d = 0; d < 3; ++d) FLABI(fl_vec_lincomb(h, c->sz[1 + d], 0., f->V[d], 0., NULL, f->V[d])); /* interprhs = 0 */
  FLABI(fl_vec_lincomb(h, N, 0., f->p, 0., NULL, f->p));                                               /* VecSet(contrhs, 0), :3046 */
  for (int b = 0; b < 6; ++b) {
    if (ns->bcs[b].type != NS_BC_VELOCITY || !cnl_touches(ns, b)) continue;
    const int        ax = b / 2, side = b % 2, a1 = ax == 0 ? 1 : 0, a2 = ax == 2 ? 1 : 2;
    const fl_decomp *D = &ns->mesh->decomp;
    const int64_t    np = D->len[a1] * D->len[a2], n = cart->N[ax];
    const double    *xf = cart->xf[ax], *xc = cart->xc[ax];
    const double    *vb0[3], *vb1[3];
    FLCHK(cnl_eval_velocity(ns, b, t, vb0));
    FLCHK(cnl_eval_velocity(ns, b, t + dt, vb1));
    /* coefficient of the wall value in the one-sided second-derivative row, :698-701 / :726-729 */
    double h1, h2, h3, hcell;
    if (n < 3) return E_SUP;
    if (!side) {
      h1 = xc[0] - xf[0]; h2 = xc[1] - xc[0]; h3 = xc[2] - xc[0]; hcell = xf[1] - xf[0];
    } else {
      h1 = xf[n] - xc[n - 1]; h2 = xc[n - 1] - xc[n - 2]; h3 = xc[n - 1] - xc[n - 3]; hcell = xf[n] - xf[n - 1];
    }
    const double cl = 2. * (h2 + h3) / (h1 * (h1 + h2) * (h1 + h3)), sgn = side ? 0.5 : -0.5;
    for (int q = 0; q < 3; ++q) {
      /* momrhs += cv (vbcL(t) + vbcL(t+dt)) - dt vbcC(t, t+dt), :2985-2998 with :698-701 and :1338 */
      double *tmp;
      FLCHK(cnl_scratch(ns, &tmp));
      for (int64_t a = 0; a < np; ++a) tmp[a] = cv * cl * (vb0[q][a] + vb1[q][a]) - dt * sgn * (vb1[q][a] * vb0[ax][a] + vb0[q][a] * vb1[ax][a]) / hcell;
      FLCHK(cnl_upload(ns, tmp, np));
      FLABI(fl_boundary_add_cells(h, b, 1., c->plane_dev, f->v + q * N));
    }
    /* interprhs on the wall faces = the wall-normal velocity at t + dt, :3003-3005 with :2178 */
    FLCHK(cnl_upload(ns, vb1[ax], np));
    FLABI(fl_boundary_set_faces(h, b, 1., c->plane_dev, f->V[ax]));
  }
  /* immersed boundary: momrhs += spread(U_target - interp(v0)) */
  if (ns->ibm) {
    FLABI(fl_ibm_interp(ns->ibm, 3, c->sol0_v, ns->ibm_U));
    FLABI(fl_vec_lincomb(h, 3 * ns->ibm_L, -1., ns->ibm_U, 1., ns->ibm_Ut, ns->ibm_U)); /* U_target - U (z = NULL: target 0) */
    FLABI(fl_ibm_spread(ns->ibm, 3, ns->ibm_U, ns->ibm_dV, f->v));
  }
  /* Boussinesq buoyancy of the active scalars as they stand when the step begins (phi^n: explicit, first order in time); nothing is launched without
   * gravity or without an active scalar.  The forcing above is formed from v0 alone: the buoyancy of the step is not anticipated at the markers. */
  FLCHK(buoyancy_add(ns, f->v));
  /* PRESSURE_OUTLET: the boundary-condition vector of G in momrhs (:2976-2984, :219-423) and the Rhie-Chow boundary terms
   * of interprhs (:3013-3044).  As written in the reference, the G vector is NOT scaled by dt/rho in momrhs. */
  {
    int     rhiechow = 0;
    double *w = c->d_v; /* 3*cells scratch: kappa (vbcG(tq) - vbcG(tp)) */
    const double tq = ns->step == 0 ? t : t - 0.5 * dt, tp = t + 0.5 * dt, kappa = dt / ns->rho;
    for (int b = 0; b < 6; ++b) {
      if (ns->bcs[b].type != NS_BC_PRESSURE_OUTLET || !cnl_touches(ns, b)) continue;
      const int        ax = b / 2, side = b % 2, a1 = ax == 0 ? 1 : 0, a2 = ax == 2 ? 1 : 2;
      const fl_decomp *D = &ns->mesh->decomp;
      const int64_t    n1 = D->len[a1], n2 = D->len[a2], np = n1 * n2, n = cart->N[ax];
      const double    *xf = cart->xf[ax], *xc = cart->xc[ax];
      if (!ns->bcs[b].pressure || n < 2) return !ns->bcs[b].pressure ? E_ARG_WRONGSTATE : E_SUP;
      double *pq, *pp, *tmp;
      FLCHK(cnl_scratch(ns, &pq));
      FLCHK(cnl_scratch(ns, &pp));
      FLCHK(cnl_scratch(ns, &tmp));
      int     differs = 0;
      for (int64_t j = 0; j < n2; ++j)
        for (int64_t i = 0; i < n1; ++i) {
          double xb[3], vq = 0., vp = 0.;
          xb[ax] = xf[side ? n : 0];
          xb[a1] = cart->xc[a1][D->lo[a1] + i];
          xb[a2] = cart->xc[a2][D->lo[a2] + j];
          FLCHK(ns->bcs[b].pressure(3, tq, xb, &vq, ns->bcs[b].ctx_pressure));
          FLCHK(ns->bcs[b].pressure(3, tp, xb, &vp, ns->bcs[b].ctx_pressure));
          pq[j * n1 + i] = vq;
          pp[j * n1 + i] = vp;
          differs |= vq != vp;
        }
      /* G: one-sided first derivative through the boundary value, :257-259 / :285-287 */
      const double h1 = side ? xf[n] - xc[n - 1] : xc[0] - xf[0], h2 = side ? xc[n - 1] - xc[n - 2] : xc[1] - xc[0];
      const double cg = (side ? 1. : -1.) * h2 / (h1 * (h1 + h2));
      FLCHK(cnl_upload(ns, pq, np));
      FLABI(fl_boundary_add_cells(h, b, -cg, c->plane_dev, f->v + ax * N)); /* VecAXPY(momrhs, -1, Gp), Gp = kappa G p + vbcG(tq) */
      if (differs) {
        /* Gst: :2641-2647 / :2669-2675 */
        const double g1 = side ? xf[n] - xc[n - 1] : xc[0] - xf[0], g2 = side ? xf[n] - xc[n - 2] : xc[1] - xf[0];
        const double cgst = (side ? 1. : -1.) * (g1 + g2) / (g1 * g2);
        if (!rhiechow) FLABI(fl_vec_lincomb(h, 3 * N, 0., w, 0., NULL, w));
        rhiechow = 1;
        for (int64_t a = 0; a < np; ++a) tmp[a] = pq[a] - pp[a];
        FLCHK(cnl_upload(ns, tmp, np));
        FLABI(fl_boundary_add_cells(h, b, kappa * cg, c->plane_dev, w + ax * N));     /* kappa (vbcGq - vbcGp), :3031-3032 */
        FLABI(fl_boundary_add_faces(h, b, kappa * cgst, c->plane_dev, f->V[ax]));     /* + kappa (vbcGstq - vbcGstp), :3034-3035 */
      }
    }
    /* MatMultAdd(negT, ...) is collective (ghost exchange of w): the ranks that do not touch an outlet, or whose part of it is steady, must take
     * the same branch as the one that found a difference -- one flag summed over the ranks, only where the problem has an outlet at all (the
     * boundary TYPES are known to every rank).  Found by the 2 x 2 x 2 run of tests/test_gpu_config5.py: rounds 1-4 never had an outlet on a
     * split axis. */
    int any_outlet = 0;
    for (int b = 0; b < 6; ++b) any_outlet |= ns->bcs[b].type == NS_BC_PRESSURE_OUTLET;
    if (any_outlet && ns->mesh->size > 1) {
      double flag = (double)rhiechow;
      FLABI(fl_poisson_allreduce_sum(h, &flag, 1));
      if (flag > 0. && !rhiechow) FLABI(fl_vec_lincomb(h, 3 * N, 0., w, 0., NULL, w)); /* this rank's share of w is zero */
      rhiechow = flag > 0.;
    }
    if (rhiechow) {
      /* interprhs += (-T) w, :3033 */
      const double *rhs[3] = {f->V[0], f->V[1], f->V[2]};
      FLABI(fl_momentum_face_interp_scaled(ns->momentum, -1., w, rhs, f->V));
    }
  }
  return 0;
}

/* NSFormJacobian_CNLinear (cnlinear.c:62-84 -> cnlinearcart3d.c:2864-2943).  NS_INIT_JACOBIAN wires the constant blocks: kappa G, -T,
 * I, -R = (-T)(kappa G) + kappa Gst, D and the composed "Laplacian" / "StaggeredGradient" (:2885-2928) -- all of them 1-D tables the
 * handle J built when it was created (fl_momentum_create); what is left to do here is to tell it PC_ABF's Ainv types.  Then, for
 * either type, "if (ns->sol0)": A = I + dt C(V0, v0interp) - (mu dt / 2 rho) L (:2930-2941), matrix-free from sol0's face-normal
 * velocity, cnl->v0interp and v0 itself (the inner faces of v0interp are formed from v0 inside the kernel). */
static FlErrorCode NSFormJacobian_CNLinear(NS ns, const NSVec *x, NSMat J, NSFormJacobianType type)
{
  NS_CNLinear *c = (NS_CNLinear *)ns->data;
  (void)x;
  if (!J) return E_ARG_NULL;
  if (type == NS_INIT_JACOBIAN) FLABI(fl_abf_set_ainv_types(J, ns->schur_ainv, ns->upper_ainv));
  if (c && c->have_sol0) {
    const double *V0[3] = {c->sol0_V[0], c->sol0_V[1], c->sol0_V[2]};
    const double *W[9];
    for (int q = 0; q < 9; ++q) W[q] = c->W[q];
    /* W = B v0 with the boundary values set on boundary faces only: the operator may form the inner ones from v0 */
    FLABI(fl_momentum_set_state_v0(J, ns->dt, ns->rho, ns->mu, V0, W, c->sol0_v));
  }
  return 0;
}

#include <time.h>
static int step_timing(void)
{
  static int on = -1;
  if (on < 0) {
    const char *e = getenv("FLUCA_STEP_TIMING");
    on = e && atoi(e) != 0;
  }
  return on;
}
static double step_clock(NS ns)
{
  struct timespec ts;
  if (ns->poisson) (void)fl_poisson_synchronize(ns->poisson);
  clock_gettime(CLOCK_MONOTONIC, &ts);
  return ts.tv_sec + 1e-9 * ts.tv_nsec;
}

/* ns->J: created at NSSetUp (MatCreateNest, nsbasic.c:203-207) where the block is large enough for the momentum rows, else here */
static FlErrorCode ns_jacobian(NS ns)
{
  if (ns->momentum) return 0;
  if (!ns->poisson) return E_ARG_WRONGSTATE;
  FLABI(fl_momentum_create(ns->poisson, &ns->momentum));
  return NSFormJacobian(ns, NULL, ns->momentum, NS_INIT_JACOBIAN);
}

static FlErrorCode NSStep_CNLinear(NS ns)
{
  NS_CNLinear *c = (NS_CNLinear *)ns->data;
  if (!c) return E_ARG_WRONGSTATE;
  fl_poisson   *h = ns->poisson;
  const int64_t N = c->sz[0];
  FLCHK(ns_jacobian(ns));
  if (!ns->bc_keep) /* -ns_keep_boundary_values false: nothing a callback returned in an earlier step is used again */
    for (int b = 0; b < 6; ++b) c->bc_have[b][0] = c->bc_have[b][1] = 0;
  const int timing = step_timing();
  double    tm[6] = {0., 0., 0., 0., 0., 0.};
  if (timing) tm[0] = step_clock(ns);
  /* -ns_abf_momentum_guess_extrapolate: 2 v^n - v^(n-1) while sol0 still holds v^(n-1); fractional step only (what reads x_v as a guess below) */
  const int guess = ns->ksp_type != 2 ? ns->mom_guess_previous : 0;
  if (guess == 2 && c->have_sol0) FLABI(fl_vec_lincomb(h, 3 * N, 2., c->sol_v, -1., c->sol0_v, c->x_v));
  else if (guess) FLABI(fl_vec_lincomb(h, 3 * N, 1., c->sol_v, 0., NULL, c->x_v));
  /* NSStep: VecCopy(sol, sol0), nsbasic.c:281-282 (the vectors are this type's device arrays, so the copy is made here) */
  FLABI(fl_vec_lincomb(h, 3 * N, 1., c->sol_v, 0., NULL, c->sol0_v));
  FLABI(fl_vec_lincomb(h, N, 1., c->sol_p, 0., NULL, c->sol0_p));
  for (int d = 0; d < 3; ++d) FLABI(fl_vec_lincomb(h, c->sz[1 + d], 1., c->sol_V[d], 0., NULL, c->sol0_V[d]));
  c->have_sol0 = 1;

  /* v0interp = B v0 + vbc(t), cnlinearcart3d.c:2826-2829; vbc: :1749-1932 */
  /* only the block-end faces are formed here: the operator forms the inner ones from v0 itself (fl_momentum_set_state_v0) */
  FLABI(fl_momentum_interp_faces_ends(ns->momentum, c->sol0_v, NULL, c->W));
  for (int b = 0; b < 6; ++b) {
    if (ns->bcs[b].type != NS_BC_VELOCITY || !cnl_touches(ns, b)) continue;
    const int        ax = b / 2, a1 = ax == 0 ? 1 : 0, a2 = ax == 2 ? 1 : 2;
    const fl_decomp *D = &ns->mesh->decomp;
    const int64_t    np = D->len[a1] * D->len[a2];
    const double    *vb0[3];
    FLCHK(cnl_eval_velocity(ns, b, ns->t, vb0));
    for (int q = 0; q < 3; ++q) { /* v0interp on the wall faces = the wall velocity at t (INSERT), :1788 */
      FLCHK(cnl_upload(ns, vb0[q], np));
      FLABI(fl_boundary_set_faces(h, b, 1., c->plane_dev, c->W[q * 3 + ax]));
    }
  }
  /* SNESSolve(ns->snes, NULL, ns->x), :2833, with SNESSetPicard (nsbasic.c:248): the right-hand side comes from the type's
   * formfunction, the operator from its formjacobian -- both through the ops table (nsbasic.c:115-131) */
  NSVec x = {c->x_v, {c->x_V[0], c->x_V[1], c->x_V[2]}, c->x_p}, f = {c->f_v, {c->f_V[0], c->f_V[1], c->f_V[2]}, c->f_p};
  if (timing) tm[1] = step_clock(ns);
  FLCHK(NSFormFunction(ns, &x, &f));
  if (timing) tm[2] = step_clock(ns);
  FLCHK(NSFormJacobian(ns, &x, ns->momentum, NS_UPDATE_JACOBIAN));
  if (timing) tm[3] = step_clock(ns);
  /* KSPSolve(J, f, x) with PC_ABF */
  fl_ksp_stats  st[2];
  const double *fV[3] = {c->f_V[0], c->f_V[1], c->f_V[2]};
  if (ns->ksp_type == 2) {
    ns->reason  = 0;
    ns->mom_its = ns->schur_its = 0;
    FLCHK(cnl_gmres(ns, &f, &x));
  } else {
    fl_ksp_opts mom1 = ns->mom;
    /* -ns_abf_momentum_guess_previous / _extrapolate: v* starts from the guess left in x_v above (the right-hand side is the whole momrhs here, not a
     * residual).  NSFormFunction and NSFormJacobian do not write x */
    if (guess) mom1.initial_guess_nonzero = 1;
    FLABI(fl_abf_apply(ns->momentum, &mom1, &ns->schur, c->f_v, fV, c->f_p, c->x_v, c->x_V, c->x_p, st));
  }
  if (ns->ksp_type != 2) {
    ns->ksp_its   = 1;
    ns->reason    = 0;
    ns->mom_its   = st[0].iters;
    ns->schur_its = st[1].iters;
  }
  /* like PETSc without -ksp_error_if_not_converged, an inner solve that stops short is not an error by itself: the outer
   * residual decides.  NaN / Inf is. */
  if (ns->ksp_type != 2 && (st[0].reason == FL_DIVERGED_NANORINF || st[1].reason == FL_DIVERGED_NANORINF)) ns->reason = -1; /* NS_DIVERGED_LINEAR_SOLVE */
  if (ns->ksp_type == 0 && ns->reason >= 0) {
    double fnorm, rnorm = 0., part;
    FLABI(fl_vec_dot(h, 3 * N, c->f_v, c->f_v, &fnorm));
    for (int d = 0; d < 3; ++d) {
      FLABI(fl_vec_dot(h, c->sz[1 + d], c->f_V[d], c->f_V[d], &part));
      fnorm += part;
    }
    FLABI(fl_vec_dot(h, N, c->f_p, c->f_p, &part));
    fnorm += part;
    fnorm = sqrt(fnorm);
    ns->ksp_rnorm0 = fnorm;
    const double ttol = ns->ksp_rtol * fnorm > ns->ksp_atol ? ns->ksp_rtol * fnorm : ns->ksp_atol;
    for (;;) {
      FLCHK(cnl_residual(ns, &rnorm));
      ns->ksp_rnorm = rnorm;
      if (!(rnorm == rnorm)) { ns->reason = -1; break; }
      if (rnorm <= ttol) break;
      if (ns->ksp_its >= ns->ksp_max_it) { ns->reason = -1; break; }
      const double *rV[3] = {c->r_V[0], c->r_V[1], c->r_V[2]};
      FLABI(fl_abf_apply(ns->momentum, &ns->mom, &ns->schur, c->r_v, rV, c->r_p, c->d_v, c->d_V, c->d_p, st));
      ns->mom_its += st[0].iters;
      ns->schur_its += st[1].iters;
      if (st[0].reason == FL_DIVERGED_NANORINF || st[1].reason == FL_DIVERGED_NANORINF) { ns->reason = -1; break; }
      FLABI(fl_vec_lincomb(h, 3 * N, 1., c->x_v, 1., c->d_v, c->x_v));
      FLABI(fl_vec_lincomb(h, N, 1., c->x_p, 1., c->d_p, c->x_p));
      for (int d = 0; d < 3; ++d) FLABI(fl_vec_lincomb(h, c->sz[1 + d], 1., c->x_V[d], 1., c->d_V[d], c->x_V[d]));
      ++ns->ksp_its;
    }
  }
  if (timing) tm[4] = step_clock(ns);
  if (ns->reason < 0) return 0; /* NSStep reports it; the solution is left untouched (NSCheckDiverged) */
  /* v, V <- x; pressure update, :2841-2854 */
  FLABI(fl_vec_lincomb(h, 3 * N, 1., c->x_v, 0., NULL, c->sol_v));
  for (int d = 0; d < 3; ++d) FLABI(fl_vec_lincomb(h, c->sz[1 + d], 1., c->x_V[d], 0., NULL, c->sol_V[d]));
  FLABI(fl_pressure_update(h, ns->step == 0, c->x_p, c->sol0_p, c->phalf, c->sol_p));
  FLABI(fl_poisson_synchronize(h));
  if (timing) {
    tm[5] = step_clock(ns);
    fprintf(stderr, "[fluca step %lld] copy sol0 + v0interp ends %.4f s | NSFormFunction %.4f | NSFormJacobian %.4f | KSPSolve (PCApply_ABF: kspA %d its, kspS %d its) %.4f | update %.4f\n",
            (long long)ns->step + 1, tm[1] - tm[0], tm[2] - tm[1], tm[3] - tm[2], ns->mom_its, ns->schur_its, tm[4] - tm[3], tm[5] - tm[4]);
  }
  return 0;
}
/* cnlinear.c:136-162 */
static FlErrorCode NSView_CNLinear(NS ns, FlucaViewer viewer)
{
  (void)ns;
  (void)viewer; /* "TODO: add view" in the reference: prints nothing */
  return 0;
}
static FlErrorCode NSViewSolution_CNLinear(NS ns, FlucaViewer viewer) /* VecView(cnl->phalf, viewer) */
{
  NS_CNLinear *c = (NS_CNLinear *)ns->data;
  if (!c) return E_ARG_WRONGSTATE;
  return viewer->ops->cellfield(viewer, ns, "PressureHalfStep", 1, c->phalf); /* the name: cnlinear.c:54 */
}
static FlErrorCode NSLoadSolution_CNLinear(NS ns, FlucaViewer viewer) /* FlucaVecLoad(cnl->phalf, viewer) */
{
  NS_CNLinear *c = (NS_CNLinear *)ns->data;
  if (!c) return E_ARG_WRONGSTATE;
  return viewer->ops->cellfield(viewer, ns, "PressureHalfStep", 1, c->phalf);
}
FlErrorCode NSGetSolverVectors(NS ns, NSVec *x, NSVec *r)
{
  if (!ns) return E_ARG_NULL;
  if (!ns->setupcalled || !ns->data) return E_ARG_WRONGSTATE;
  NS_CNLinear *c = (NS_CNLinear *)ns->data;
  if (x) {
    x->v = c->x_v;
    x->p = c->x_p;
    for (int d = 0; d < 3; ++d) x->V[d] = c->x_V[d];
  }
  if (r) {
    r->v = c->f_v;
    r->p = c->f_p;
    for (int d = 0; d < 3; ++d) r->V[d] = c->f_V[d];
  }
  return 0;
}

FlErrorCode NSCreate_CNLinear(NS ns) /* cnlinear.c:164-187 */
{
  ns->ops->setfromoptions = NULL; /* NSSetFromOptions_CNLinear (cnlinear.c:7-11) reads no option */
  ns->ops->setup          = NSSetUp_CNLinear;
  ns->ops->step           = NSStep_CNLinear;
  ns->ops->formjacobian   = NSFormJacobian_CNLinear;
  ns->ops->formfunction   = NSFormFunction_CNLinear;
  ns->ops->destroy        = NSDestroy_CNLinear;
  ns->ops->view           = NSView_CNLinear;
  ns->ops->viewsolution   = NSViewSolution_CNLinear;
  ns->ops->loadsolution   = NSLoadSolution_CNLinear;
  return 0;
}
