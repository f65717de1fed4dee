// fl_buoyancy.hip -- the Boussinesq term of the momentum right-hand side, for all active scalars in ONE streaming pass:
//     momrhs[d N + c] += dt sum_{s < ns} a[d][s] (phi_s[c] - ref_s),     a[d][s] = -beta_s g_d
// Every phi_s is read once (non-temporal: nothing reads it again before the scalar step), every component of momrhs with a non-zero coefficient is
// read and written once, a component whose coefficients are all zero is not touched: 8 ns + 16 (active components) bytes per cell.
// A lane owns two adjacent cells of the flat arrays (the term is pointwise: no rows) with 16-byte accesses; the coefficient table, the references and
// the pointers are kernel arguments (scalar loads).  One block of eight waves per CU, grid-stride, never a second round of blocks.
// The arrays are the callers' unpadded ones: component d starts at momrhs + d N, 8 bytes off a 16-byte boundary when d N is odd -- such a component
// (and a phi that is not 16-byte aligned) is accessed with two 8-byte accesses per lane instead, the pairs of cells stay the same.
// Operation order per cell and component (pinned by tests/test_gpu_buoyancy.py): x_s = phi_s - ref_s; t = a_0 x_0; t = fma(a_s, x_s, t), s = 1 ..;
// momrhs = fma(dt, t, momrhs).
#include "fl_device.h"
#include "fl_mom_handle.h"

namespace fl {

typedef double dbl2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ dbl2 by_load(const double *p, int64_t c, bool vec, bool two)
{
  if (vec && two) return *reinterpret_cast<const dbl2 *>(p + c);
  dbl2 r;
  r.x = p[c];
  r.y = two ? p[c + 1] : 0.;
  return r;
}
__device__ __forceinline__ dbl2 by_load_nt(const double *p, int64_t c, bool vec, bool two)
{
  if (vec && two) return __builtin_nontemporal_load(reinterpret_cast<const dbl2 *>(p + c));
  dbl2 r;
  r.x = __builtin_nontemporal_load(p + c);
  r.y = two ? __builtin_nontemporal_load(p + c + 1) : 0.;
  return r;
}
__device__ __forceinline__ void by_store(double *p, int64_t c, bool vec, bool two, dbl2 v)
{
  if (vec && two) {
    *reinterpret_cast<dbl2 *>(p + c) = v;
    return;
  }
  p[c] = v.x;
  if (two) p[c + 1] = v.y;
}

// act: bit d = component d has a non-zero coefficient; vec: bit d = momrhs + d N is 16-byte aligned, bit 3 + s = phi_s is
__global__ void __launch_bounds__(BUOY_THREADS) k_buoyancy(int64_t N, int ns, int act, int vec, BuoyArgs A, double dt, double *momrhs)
{
  const int64_t npair = (N + 1) >> 1;
  for (int64_t q = (int64_t)blockIdx.x * BUOY_THREADS + threadIdx.x; q < npair; q += (int64_t)gridDim.x * BUOY_THREADS) {
    const int64_t c = 2 * q;
    const bool    two = c + 1 < N;
    // momrhs first: its loads are in flight while the sum is formed
    dbl2 m[3];
#pragma unroll
    for (int d = 0; d < 3; ++d)
      if ((act >> d) & 1) m[d] = by_load(momrhs + d * N, c, (vec >> d) & 1, two);
    dbl2 t[3];
#pragma unroll
    for (int s = 0; s < BUOY_MAXS; ++s) {
      if (s < ns) {
        const dbl2 x = by_load_nt(A.phi[s], c, (vec >> (3 + s)) & 1, two) - A.ref[s];
#pragma unroll
        for (int d = 0; d < 3; ++d) {
          if (!((act >> d) & 1)) continue;
          const double a = A.a[d][s];
          if (s == 0) t[d] = a * x;
          else {
            t[d].x = fma(a, x.x, t[d].x);
            t[d].y = fma(a, x.y, t[d].y);
          }
        }
      }
    }
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      if (!((act >> d) & 1)) continue;
      dbl2 r;
      r.x = fma(dt, t[d].x, m[d].x);
      r.y = fma(dt, t[d].y, m[d].y);
      by_store(momrhs + d * N, c, (vec >> d) & 1, two, r);
    }
  }
}

int device_cus(int device)
{
  static int known[64] = {};  // (written with the same value by whichever thread asks first)
  if (device < 0 || device >= 64) return 0;
  if (!known[device]) {
    int n = 0;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || n < 1) return 0;
    known[device] = n;
  }
  return known[device];
}

// One block per CU of the device (256 where the runtime does not say), no more than the pairs need.  Host arithmetic only.
int buoyancy_blocks(int64_t N, int ncu)
{
  const int64_t npair = (N + 1) / 2;
  return (int)std::max<int64_t>(1, std::min<int64_t>((npair + BUOY_THREADS - 1) / BUOY_THREADS, ncu > 0 ? ncu : 256));
}

void launch_buoyancy(hipStream_t st, int nblocks, int64_t N, int ns, int act, const BuoyArgs &A, double dt, double *momrhs)
{
  int vec = 0;
  for (int d = 0; d < 3; ++d)
    if ((reinterpret_cast<uintptr_t>(momrhs + d * N) & 15) == 0) vec |= 1 << d;
  for (int s = 0; s < ns; ++s)
    if ((reinterpret_cast<uintptr_t>(A.phi[s]) & 15) == 0) vec |= 1 << (3 + s);
  hipLaunchKernelGGL(k_buoyancy, dim3(nblocks), dim3(BUOY_THREADS), 0, st, N, ns, act, vec, A, dt, momrhs);
}

}  // namespace fl

using namespace fl;

// momrhs += dt sum_s a_s (phi_s - ref_s): the Boussinesq term, one launch for all scalars.  No reference counterpart.  Every argument is checked
// before the handle is read.
extern "C" int fl_momentum_add_buoyancy(fl_momentum *m, int nscalar, const double *const phi_dev[], const double accel[], const double phi_ref[], double dt, double *momrhs_dev)
{
  if (!m || !phi_dev || !accel || !phi_ref || !momrhs_dev) return FL_ERR_ARG_NULL;
  if (nscalar < 1 || nscalar > BUOY_MAXS || !std::isfinite(dt)) return FL_ERR_ARG_OUTOFRANGE;
  BuoyArgs A;
  std::memset(&A, 0, sizeof(A));
  int act = 0;
  for (int s = 0; s < nscalar; ++s) {
    if (!phi_dev[s]) return FL_ERR_ARG_NULL;
    if (!std::isfinite(phi_ref[s])) return FL_ERR_ARG_OUTOFRANGE;
    A.phi[s] = phi_dev[s];
    A.ref[s] = phi_ref[s];
    for (int d = 0; d < 3; ++d) {
      if (!std::isfinite(accel[3 * s + d])) return FL_ERR_ARG_OUTOFRANGE;
      A.a[d][s] = accel[3 * s + d];
      if (accel[3 * s + d] != 0.) act |= 1 << d;
    }
  }
  if (!act) return FL_SUCCESS;  // nothing to add: no launch
  fl_poisson *h = m->p;  // of the handle only the borrowed grid is needed
  FL_HIP(hipSetDevice(h->device));
  launch_buoyancy(h->stream, buoyancy_blocks(h->ncell, device_cus(h->device)), h->ncell, nscalar, act, A, dt, momrhs_dev);
  FL_HIP(hipGetLastError());
  return FL_SUCCESS;
}

// Not part of the public C-ABI (tests): the launch of k_buoyancy on N cells -- 0 blocks, 1 threads per block, 2 cells per lane and trip (so the
// product of the three is one round of the grid-stride loop).
extern "C" int fldbg_buoyancy_plan(int device, int64_t ncell, int *out, int nout)
{
  if (ncell < 1) return FL_ERR_ARG_OUTOFRANGE;
  if (!out) return 3;
  if (nout < 3) return FL_ERR_ARG_SIZ;
  out[0] = fl::buoyancy_blocks(ncell, fl::device_cus(device));
  out[1] = fl::BUOY_THREADS;
  out[2] = 2;
  return 3;
}
