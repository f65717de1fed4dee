/*
 * heated_cavity_3d.c -- the differentially heated cavity (natural convection, Boussinesq) against the C host mirror (include/fluca_host.h):
 * hot wall at x = 0 (T = 1), cold wall at x = 1 (T = 0), insulated floor and ceiling, periodic and thin in z, gravity along -y.  The temperature is
 * a scalar of NSAddScalar made active by NSSetScalarBuoyancy; the heat flux through the hot wall comes from NSGetScalarBoundaryFlux.
 * In units of the box width, the temperature difference and the free-fall velocity sqrt(g beta dT L):  nu = sqrt(Pr / Ra), alpha = 1 / sqrt(Ra Pr),
 * g beta = 1, and the Nusselt number of a wall is its total flux (convective + diffusive, along +x) over alpha x wall area.
 * -implicit: the temperature's diffusion by backward Euler (NSSetScalarImplicit, theta = 1), a fixed number of Chebyshev launches per step that is printed
 * beside the Courant numbers: the diffusive one then no longer limits the step (try -cart_grid_x 128 -cart_grid_y 128 with and without it).
 * A demonstration, not a test: no number printed here is asserted anywhere.  One rank.
 *
 *   gcc -O2 examples/heated_cavity_3d.c -Iinclude -Lfluca_amd/lib -lfluca_host -lflucahip -lm -Wl,-rpath,$PWD/fluca_amd/lib
 *   ./a.out -cart_grid_x 64 -cart_grid_y 64 -cart_grid_z 4 -Ra 1e5 -Pr 0.71 -ns_time_step_size 2e-2 -ns_max_steps 200
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "fluca_host.h"

#define CHK(call)                                                                 \
  do {                                                                            \
    FlErrorCode e_ = (call);                                                      \
    if (e_) {                                                                     \
      fprintf(stderr, "%s:%d: %s -> error %d\n", __FILE__, __LINE__, #call, e_); \
      return 1;                                                                   \
    }                                                                             \
  } while (0)
#define ABI(call) CHK(-(call))

static FlErrorCode wall_velocity(int dim, double t, const double x[], double val[], void *ctx)
{
  (void)dim; (void)t; (void)x; (void)ctx;
  val[0] = val[1] = val[2] = 0.;
  return 0;
}

int main(int argc, char **argv)
{
  Mesh    mesh;
  NS      ns;
  double  Ra = 1e5, Pr = 0.71;
  int64_t maxsteps = 50, step = 0;
  int     implicit = 0;
  for (int a = 1; a < argc; ++a)
    if (!strcmp(argv[a], "-implicit")) implicit = 1;
  for (int a = 1; a + 1 < argc; ++a) {
    if (!strcmp(argv[a], "-Ra")) Ra = atof(argv[a + 1]);
    if (!strcmp(argv[a], "-Pr")) Pr = atof(argv[a + 1]);
    if (!strcmp(argv[a], "-ns_max_steps")) maxsteps = atoll(argv[a + 1]);
  }
  const double nu = sqrt(Pr / Ra), alpha = 1. / sqrt(Ra * Pr);

  CHK(MeshCartCreate3d(MESHCART_BOUNDARY_NONE, MESHCART_BOUNDARY_NONE, MESHCART_BOUNDARY_PERIODIC, 32, 32, 4, 1, 1, 1, NULL, NULL, NULL, &mesh));
  CHK(MeshSetFromOptions(mesh, argc, argv));
  CHK(MeshSetUp(mesh));
  int64_t M, N, P;
  CHK(MeshCartGetGlobalSizes(mesh, &M, &N, &P));
  const double Lz = (double)P / (double)M; /* cubic cells */
  CHK(MeshCartSetUniformCoordinates(mesh, 0., 1., 0., 1., 0., Lz));

  CHK(NSCreate(&ns));
  CHK(NSSetType(ns, NSCNLINEAR));
  CHK(NSSetMesh(ns, mesh));
  CHK(NSSetDensity(ns, 1.));
  CHK(NSSetViscosity(ns, nu));
  {
    NSBoundaryCondition wallbc = {.type = NS_BC_VELOCITY, .velocity = wall_velocity}, perbc = {.type = NS_BC_PERIODIC};
    for (int b = 0; b < 4; ++b) CHK(NSSetBoundaryCondition(ns, b, wallbc));
    for (int b = 4; b < 6; ++b) CHK(NSSetBoundaryCondition(ns, b, perbc));
  }
  CHK(NSSetTimeStepSize(ns, 2e-2));
  const double g[3] = {0., -1., 0.};
  CHK(NSSetGravity(ns, g)); /* -ns_gravity gx,gy,gz overrides it */
  CHK(NSSetFromOptions(ns, argc, argv));
  CHK(NSSetUp(ns));

  /* the temperature: Dirichlet 1 / 0 on the hot / cold wall, Neumann 0 (the default) on floor and ceiling; beta = 1 about the mean temperature */
  int     T;
  double *T_dev;
  CHK(NSAddScalar(ns, "temperature", alpha, "vanleer", &T));
  CHK(NSSetScalarBoundaryCondition(ns, T, 0, 0, 1.));
  CHK(NSSetScalarBoundaryCondition(ns, T, 1, 0, 0.));
  CHK(NSSetScalarBuoyancy(ns, T, 1., 0.5));
  if (implicit) CHK(NSSetScalarImplicit(ns, T, 1., 1e-6));
  CHK(NSGetScalarArray(ns, T, &T_dev));
  {
    /* the conduction profile: the flow starts from rest and the walls' fluxes start at alpha x area (Nu = 1) */
    double *h = (double *)malloc(sizeof(double) * (size_t)(M * N * P));
    if (!h) return 1;
    for (int64_t c = 0; c < M * N * P; ++c) h[c] = 1. - ((double)(c % M) + 0.5) / (double)M;
    ABI(fl_memcpy_h2d(0, T_dev, h, sizeof(double) * (size_t)(M * N * P)));
    free(h);
  }
  CHK(NSView(ns, NULL));

  printf("Ra %g  Pr %g  nu %g  alpha %g  grid %lld x %lld x %lld\n", Ra, Pr, nu, alpha, (long long)M, (long long)N, (long long)P);
  while (step < maxsteps) {
    int    its, reason;
    double rnorm, t, flux[12], cfl[2];
    CHK(NSStep(ns));
    CHK(NSGetTimeStep(ns, &step));
    CHK(NSGetTime(ns, &t));
    CHK(NSGetLinearSolveInfo(ns, &its, &rnorm, &reason));
    if (reason < 0) {
      fprintf(stderr, "step %lld failed\n", (long long)step);
      return 2;
    }
    if (step % 10 && step != maxsteps) continue;
    CHK(NSGetScalarBoundaryFlux(ns, T, flux));
    CHK(NSGetScalarCFL(ns, T, cfl));
    /* both along +x: heat enters through the hot wall (boundary 0) and leaves through the cold one (boundary 1) */
    int    cheb = 0;
    double bound = 1.;
    CHK(NSGetScalarImplicitInfo(ns, T, &cheb, &bound));
    printf("%lld NS time %g  outer its %d  Nu hot wall %.6f  Nu cold wall %.6f  scalar CFL %.3f / %.3f", (long long)step, t, its, (flux[0] + flux[1]) / (alpha * Lz),
           (flux[2] + flux[3]) / (alpha * Lz), cfl[0], cfl[1]);
    if (implicit) printf("  Chebyshev steps %d (error bound %.1e)", cheb, bound);
    printf("\n");
  }
  CHK(MeshDestroy(&mesh));
  CHK(NSDestroy(&ns));
  return 0;
}
