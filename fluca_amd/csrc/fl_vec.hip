// fl_vec.hip -- device BLAS-1 for hosts that drive an outer iteration over device vectors without a vector library of their own (the C host mirror),
// and for the host-driven loops of the library itself (GMRES on the momentum block, FGMRES on the variable-coefficient Schur complement).
#include "fl_device.h"
#include "fl_mom_handle.h"

namespace fl {

struct Vec8 {
  const double *p[8];
};
struct Coef8 {
  double a[8];
};
// VecMDot / VecMAXPY on up to 8 vectors per launch: x is read once for all of them
// partial[i * stride + block] = sum over the block's elements of x * y_i
__global__ void __launch_bounds__(256) k_mdot8(int64_t n, const double *__restrict__ x, Vec8 Y, int k, double *__restrict__ partial, int stride)
{
  __shared__ double red[8 * 4];
  double            acc[8] = {0., 0., 0., 0., 0., 0., 0., 0.};
  for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < n; q += (int64_t)gridDim.x * blockDim.x) {
    const double xv = x[q];
#pragma unroll
    for (int i = 0; i < 8; ++i)
      if (i < k) acc[i] += xv * Y.p[i][q];
  }
  block_sum<8>(acc, red);
  if (threadIdx.x == 0)
#pragma unroll
    for (int i = 0; i < 8; ++i) partial[(int64_t)i * stride + blockIdx.x] = acc[i];
}
// x += sum_i a_i y_i
__global__ void __launch_bounds__(256) k_maxpy8(int64_t n, double *__restrict__ x, Coef8 A, Vec8 Y, int k)
{
  for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < n; q += (int64_t)gridDim.x * blockDim.x) {
    double t = x[q];
#pragma unroll
    for (int i = 0; i < 8; ++i)
      if (i < k) t += A.a[i] * Y.p[i][q];
    x[q] = t;
  }
}
// y = a x + b z (z may be NULL; y may alias x or z)
__global__ void __launch_bounds__(256) k_lincomb(int64_t n, double a, const double *x, double b, const double *z, double *y)
{
  // a zero coefficient means "not part of the sum": the vector is not read (VecSet(y, 0) as 0 x + 0 z must not keep a NaN of x alive, nor pay for reading it)
  const bool ux = a != 0., uz = z && b != 0.;
  for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < n; q += (int64_t)gridDim.x * blockDim.x) y[q] = (ux ? a * x[q] : 0.) + (uz ? b * z[q] : 0.);
}

// partial[block] = sum over this block's grid-stride share of x[q] y[q]
__global__ void __launch_bounds__(256) k_dot(int64_t n, const double *__restrict__ x, const double *__restrict__ y, double *__restrict__ partial)
{
  __shared__ double red[4];
  double            v[1] = {0.};
  for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < n; q += (int64_t)gridDim.x * blockDim.x) v[0] += x[q] * y[q];
  block_sum<1>(v, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = v[0];
}

void lincomb(fl_poisson *h, int64_t n, double a, const double *x, double b, const double *z, double *y)
{
  hipLaunchKernelGGL(k_lincomb, dim3(nblk_flat(n)), dim3(256), 0, h->stream, n, a, x, b, z, y);
}

}  // namespace fl

using namespace fl;

extern "C" int fl_vec_lincomb(fl_poisson *h, int64_t n, double a, const double *x_dev, double b, const double *z_dev, double *y_dev)
{
  if (!h || !x_dev || !y_dev) return FL_ERR_ARG_NULL;
  if (n < 0) return FL_ERR_ARG_OUTOFRANGE;
  FL_HIP(hipSetDevice(h->device));
  if (n > 0) lincomb(h, n, a, x_dev, b, z_dev, y_dev);
  FL_HIP(hipGetLastError());
  return FL_SUCCESS;
}

extern "C" int fl_vec_dot(fl_poisson *h, int64_t n, const double *x_dev, const double *y_dev, double *result)
{
  if (!h || !x_dev || !y_dev || !result) return FL_ERR_ARG_NULL;
  if (n < 0) return FL_ERR_ARG_OUTOFRANGE;
  FL_HIP(hipSetDevice(h->device));
  FL_CHK(fl_ensure_partials(h, 1024));
  const int nb = (int)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, 1024));
  hipLaunchKernelGGL(k_dot, dim3(nb), dim3(256), 0, h->stream, n, x_dev, y_dev, h->partial);
  launch_reduce(h->stream, h->partial, nb, h->partial_stride, 1, h->sums);
  if (h->multi) FL_CHK(h->comm.allreduce(h->stream, h->sums, NSLOT));   // every rank holds its OWNED entries only
  FL_HIP(hipMemcpyAsync(result, h->sums, sizeof(double), hipMemcpyDeviceToHost, h->stream));
  FL_HIP(hipStreamSynchronize(h->stream));
  return FL_SUCCESS;
}

// VecMDot: out[i] = x . y_i for i < k, summed over all ranks; one host wait for all k
extern "C" int fl_vec_mdot(fl_poisson *h, int64_t n, const double *x_dev, const double *const *ys_dev, int k, double *out)
{
  if (!h || !x_dev || !ys_dev || !out) return FL_ERR_ARG_NULL;
  if (n < 0 || k < 0) return FL_ERR_ARG_OUTOFRANGE;
  FL_HIP(hipSetDevice(h->device));
  FL_CHK(fl_ensure_partials(h, 1024));
  const int nb = (int)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, 1024));
  for (int i0 = 0; i0 < k; i0 += 8) {
    const int kk = std::min(8, k - i0);
    Vec8      Y;
    for (int i = 0; i < 8; ++i) {
      Y.p[i] = i < kk ? ys_dev[i0 + i] : x_dev;
      if (!Y.p[i]) return FL_ERR_ARG_NULL;
    }
    hipLaunchKernelGGL(k_mdot8, dim3(nb), dim3(256), 0, h->stream, n, x_dev, Y, kk, h->partial, h->partial_stride);
    launch_reduce(h->stream, h->partial, nb, h->partial_stride, 8, h->sums);
    if (h->multi) FL_CHK(h->comm.allreduce(h->stream, h->sums, NSLOT));
    FL_HIP(hipMemcpyAsync(out + i0, h->sums, sizeof(double) * kk, hipMemcpyDeviceToHost, h->stream));
  }
  FL_HIP(hipStreamSynchronize(h->stream));
  return FL_SUCCESS;
}

// VecMAXPY: x += sum_i alpha_i y_i
extern "C" int fl_vec_maxpy(fl_poisson *h, int64_t n, double *x_dev, const double *alphas, const double *const *ys_dev, int k)
{
  if (!h || !x_dev || !ys_dev || !alphas) return FL_ERR_ARG_NULL;
  if (n < 0 || k < 0) return FL_ERR_ARG_OUTOFRANGE;
  FL_HIP(hipSetDevice(h->device));
  for (int i0 = 0; i0 < k && n > 0; i0 += 8) {
    const int kk = std::min(8, k - i0);
    Vec8      Y;
    Coef8     A;
    for (int i = 0; i < 8; ++i) {
      Y.p[i] = i < kk ? ys_dev[i0 + i] : x_dev;
      A.a[i] = i < kk ? alphas[i0 + i] : 0.;
      if (!Y.p[i]) return FL_ERR_ARG_NULL;
    }
    hipLaunchKernelGGL(k_maxpy8, dim3(nblk_flat(n)), dim3(256), 0, h->stream, n, x_dev, A, Y, kk);
  }
  FL_HIP(hipGetLastError());
  return FL_SUCCESS;
}
