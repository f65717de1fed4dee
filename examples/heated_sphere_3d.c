/*
 * heated_sphere_3d.c -- a heated sphere in a channel cross-flow: the channel-plus-sphere set-up of flow_configs.c (-config sphere: parabolic VELOCITY
 * inlet, PRESSURE_OUTLET p = 0, no-slip walls, periodic span, a sphere of diameter N/8 cells at the centre held at rest by direct forcing) with one
 * scalar, the temperature, held at 1 on the sphere's markers (NSSetScalarImmersedBoundary) and at 0 at the inlet.  Per step it prints the heat rate
 * NSGetScalarImmersedBoundaryRate returns -- the scalar content per unit time the sphere hands to the fluid -- and the Nusselt number that rate
 * makes with the conduction scale, Nu = rate / (alpha (T_s - T_in) 4 pi R^2 / D).  With -ns_gravity gx,gy,gz the temperature drives the flow
 * (beta = 1 about T = 0): the plume.  The number is one to watch over a few steps, not one to quote: the start is impulsive and only the surface
 * markers are held, not the sphere's interior.
 *
 *   ./a.out -n 64 -Re 100 -Pr 0.71 -ns_max_steps 5 [-ns_scalar_ibm_passes 3] [-ns_scalar_implicit_theta 1] [-ns_gravity 0,-1,0]
 *
 *   gcc -O2 examples/heated_sphere_3d.c -Iinclude -Lfluca_amd/lib -lfluca_host -lflucahip -lm -Wl,-rpath,$PWD/fluca_amd/lib
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

static FlErrorCode zero_velocity(int dim, double t, const double x[], double val[], void *ctx)
{
  (void)dim; (void)t; (void)x; (void)ctx;
  val[0] = val[1] = val[2] = 0.;
  return 0;
}
static FlErrorCode inlet_velocity(int dim, double t, const double x[], double val[], void *ctx)
{
  (void)dim; (void)t; (void)ctx;
  val[0] = 4. * x[1] * (1. - x[1]);
  val[1] = val[2] = 0.;
  return 0;
}
static FlErrorCode outlet_pressure(int dim, double t, const double x[], double val[], void *ctx)
{
  (void)dim; (void)t; (void)x; (void)ctx;
  val[0] = 0.;
  return 0;
}
static const char *opt(int argc, char **argv, const char *name, const char *dflt)
{
  for (int a = 1; a + 1 < argc; ++a)
    if (!strcmp(argv[a], name)) return argv[a + 1];
  return dflt;
}

int main(int argc, char **argv)
{
  const int64_t N = atoll(opt(argc, argv, "-n", "64")), steps = atoll(opt(argc, argv, "-ns_max_steps", "3"));
  const double  Re = atof(opt(argc, argv, "-Re", "100")), Pr = atof(opt(argc, argv, "-Pr", "0.71")), mu = 1. / Re, alpha = 1. / (Re * Pr);
  const double  PI = 3.14159265358979323846, h = 1. / (double)N, R = (double)N / 16. * h;
  Mesh          mesh;
  NS            ns;
  CHK(MeshCartCreate3d(MESHCART_BOUNDARY_NONE, MESHCART_BOUNDARY_NONE, MESHCART_BOUNDARY_PERIODIC, N, N, N, FL_DECIDE, FL_DECIDE, FL_DECIDE, NULL, NULL, NULL, &mesh));
  CHK(MeshSetUp(mesh));
  CHK(MeshCartSetUniformCoordinates(mesh, 0., 1., 0., 1., 0., 1.));
  CHK(NSCreate(&ns));
  CHK(NSSetType(ns, NSCNLINEAR));
  CHK(NSSetMesh(ns, mesh));
  CHK(NSSetDensity(ns, 1.));
  CHK(NSSetViscosity(ns, mu));
  {
    NSBoundaryCondition wall = {.type = NS_BC_VELOCITY, .velocity = zero_velocity}, in = {.type = NS_BC_VELOCITY, .velocity = inlet_velocity},
                        out = {.type = NS_BC_PRESSURE_OUTLET, .pressure = outlet_pressure}, per = {.type = NS_BC_PERIODIC};
    CHK(NSSetBoundaryCondition(ns, 0, in)); CHK(NSSetBoundaryCondition(ns, 1, out)); CHK(NSSetBoundaryCondition(ns, 2, wall));
    CHK(NSSetBoundaryCondition(ns, 3, wall)); CHK(NSSetBoundaryCondition(ns, 4, per)); CHK(NSSetBoundaryCondition(ns, 5, per));
  }
  const double dt = 0.5 / (double)N; /* CFL ~ 0.5 on the unit inflow */
  CHK(NSSetTimeStepSize(ns, dt));
  CHK(NSSetMaxSteps(ns, steps));
  CHK(NSSetFromOptions(ns, argc, argv));
  CHK(NSSetUp(ns));
  /* the sphere: markers on a Fibonacci lattice, one per h^2 of surface; marker volume h^3 */
  const int64_t L = (int64_t)llround(4. * PI * R * R / (h * h));
  double       *X = (double *)malloc(sizeof(double) * 4 * (size_t)L);
  if (!X) return 1;
  for (int64_t l = 0; l < L; ++l) {
    const double z = 1. - 2. * ((double)l + 0.5) / (double)L, r = sqrt(1. - z * z), th = PI * (3. - sqrt(5.)) * (double)l;
    X[l]         = 0.5 + R * r * cos(th);
    X[L + l]     = 0.5 + R * r * sin(th);
    X[2 * L + l] = 0.5 + R * z;
    X[3 * L + l] = h * h * h;
  }
  void *Xd = NULL;
  ABI(fl_malloc(0, sizeof(double) * 4 * (size_t)L, &Xd));
  ABI(fl_memcpy_h2d(0, Xd, X, sizeof(double) * 4 * (size_t)L));
  free(X);
  const double *D = (const double *)Xd;
  CHK(NSSetImmersedBoundary(ns, FL_DELTA_PESKIN4, L, D, D + L, D + 2 * L, D + 3 * L, NULL));
  /* the temperature: 0 at the inlet (Dirichlet), zero gradient at the outlet and the walls, 1 on the sphere */
  int T;
  CHK(NSAddScalar(ns, "temperature", alpha, "vanleer", &T));
  CHK(NSSetScalarBoundaryCondition(ns, T, 0, 0, 0.));
  for (int b = 1; b < 4; ++b) CHK(NSSetScalarBoundaryCondition(ns, T, b, 1, 0.));
  CHK(NSSetScalarBuoyancy(ns, T, 1., 0.)); /* acts only with -ns_gravity */
  const double hot = 1.;
  CHK(NSSetScalarImmersedBoundary(ns, T, -1, &hot)); /* -ns_scalar_ibm_passes */
  printf("heated sphere  cells %lld^3  dt %g  Re %g  Pr %g  alpha %g  markers %lld  R %g\n", (long long)N, dt, Re, Pr, alpha, (long long)L, R);
  for (int64_t s = 0; s < steps; ++s) {
    int    its, reason;
    double rnorm, rate;
    CHK(NSStep(ns));
    CHK(NSGetLinearSolveInfo(ns, &its, &rnorm, &reason));
    if (reason < 0) {
      fprintf(stderr, "step %lld failed\n", (long long)(s + 1));
      return 2;
    }
    CHK(NSGetScalarImmersedBoundaryRate(ns, T, &rate));
    printf("step %lld  outer its %d  heat rate %+.6e  Nu %.4f\n", (long long)(s + 1), its, rate, rate / (alpha * hot * 4. * PI * R * R / (2. * R)));
    fflush(stdout);
  }
  CHK(NSDestroy(&ns));
  CHK(MeshDestroy(&mesh));
  ABI(fl_free(0, Xd));
  return 0;
}
