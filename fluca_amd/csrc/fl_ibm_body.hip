// fl_ibm_body.hip -- per-body quantities of a marker set (fl_ibm.hip's header): force and torque on each body as sums whose bits
// depend on no order (fl_ibm_force), the Dirichlet forcing of a scalar held on the markers and the heat rate it hands over (fl_ibm_scalar_force,
// fl_ibm_scalar_rate; include/fluca_hip_ibm_scalar.h).
#include "fl_ibm_handle.h"
#include "../../include/fluca_hip_ibm_scalar.h"

namespace fl {

// ---- force and torque on each body (fl_ibm_force) -----------------------------------------------------------------------------------------
// force_b = sum_l F_l dV_l, torque_b = sum_l (r_l x F_l) dV_l over the markers of body b, r_l = X_l - about_b (minimum image on a periodic axis),
// as a sum whose bits do not depend on the order of the markers or on how they are shared out between ranks:
//   terms    every product, difference and quotient rounded once, never contracted into a fused multiply-add (force_terms)
//   max pass amax = max |t| over a group (the 3 nbody force sums; the 3 nbody torque sums), a non-finite term counts as +inf; E: amax < 2^E
//   split    t = a 2^(E-30) + b 2^(E-60) + tail, a = rint(t / 2^(E-30)), b = rint((t - a 2^(E-30)) / 2^(E-60)): integers of at most 31 bits, so
//            that sums of fewer than 2^22 of them are exact in a double in ANY order; |tail| <= 2^(E-61)
//   result   (sum a) 2^(E-30) + (sum b) 2^(E-60), the one rounding of the whole sum, formed on the host (force_combine)
// Where 2^(E-60) would be subnormal (E < -900) the group is scaled by 2^FORCE_UP, an exact operation, and the result scaled back.
constexpr int FORCE_MAXBLK = 64;   // blocks of 256 per pass: the grid-stride loop covers the rest, no second round of blocks
constexpr int FORCE_MAXBODY = 64;
constexpr int FORCE_UP = 200;
// workspace (doubles): header { amax force, amax torque, bad body id, spare }, the 12 nbody sums, about, the max pass' block partials, the slabs
constexpr int FW_SUMS = 4, FW_ABOUT = FW_SUMS + 12 * FORCE_MAXBODY, FW_PART = FW_ABOUT + 3 * FORCE_MAXBODY, FW_SLAB = FW_PART + 4 * FORCE_MAXBLK,
              FW_END = FW_SLAB + FORCE_MAXBLK * 12 * FORCE_MAXBODY;

struct ForceP {
  int64_t L;
  int     nbody;
  int     periodic[3];
  double  per[3];    // period of a periodic axis: xf[n] - xf[0]
  double  about[3];  // one body (no body array): the reference point, so that nothing is indexed
};

// the six terms of marker l: F_c dV and ((r x F)_c) dV
__device__ __forceinline__ void force_terms(const ForceP &Q, const double *__restrict__ X, const double *__restrict__ Y, const double *__restrict__ Z, const double *__restrict__ F, const double *__restrict__ dV, int64_t l,
                                            const double *ab, double t[6])
{
#pragma clang fp contract(off)
  const double pos[3] = {X[l], Y[l], Z[l]};
  const double f[3]   = {F[l], F[Q.L + l], F[2 * Q.L + l]};
  const double dv     = dV[l];
  double       r[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    r[d] = pos[d] - ab[d];
    if (Q.periodic[d]) {
      const double q = rint(r[d] / Q.per[d]);
      const double s = Q.per[d] * q;
      r[d]           = r[d] - s;
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int    c1 = (c + 1) % 3, c2 = (c + 2) % 3;
    const double p1 = r[c1] * f[c2], p2 = r[c2] * f[c1];
    const double cr = p1 - p2;
    t[c]            = f[c] * dv;
    t[3 + c]        = cr * dv;
  }
}
__device__ __forceinline__ double force_mag(double t)
{
  const double a = fabs(t);
  return a <= 1.7976931348623157e308 ? a : __builtin_inf();  // NaN fails the comparison too: fmax would drop it
}
// amax -> the exponents of the split: a = rint(t 2^sa), rem = t 2^up - a 2^ea, b = rint(rem 2^sb); live: the group has a finite, non-zero term
struct ForceSplit {
  int live, up, sa, ea, sb;
};
__host__ __device__ inline ForceSplit force_split(double amax)
{
  ForceSplit s = {0, 0, 0, 0, 0};
  if (!(amax > 0.) || !(amax <= 1.7976931348623157e308)) return s;
  const int E = ilogb(amax) + 1;  // amax < 2^E
  s.live      = 1;
  s.up        = E < -900 ? FORCE_UP : 0;
  s.sa        = 30 - E;
  s.ea        = E + s.up - 30;
  s.sb        = 60 - E - s.up;
  return s;
}
// the value of a group's sum from its two exact integer sums
static double force_combine(double amax, double A, double B)
{
  if (!(amax <= 1.7976931348623157e308)) return std::nan("");
  const ForceSplit s = force_split(amax);
  if (!s.live) return 0.;
  return std::ldexp(std::ldexp(A, s.ea) + std::ldexp(B, s.ea - 30), -s.up);
}

// Hand-off of block partials to the last-arriving block, as k_cg_Bq's (fl_kernels.hip, fused_fin): agent-scope (write-through) stores, every
// storing wave drains them, the block meets, one lane draws a ticket; the block that draws the last one reads every partial with agent-scope
// loads.  The counter is zeroed by the caller before every launch.
__device__ __forceinline__ bool force_last_block(unsigned *counter, int *flag)
{
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned t = __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    *flag            = (t == gridDim.x - 1u);
  }
  __syncthreads();
  return *flag != 0;
}

// max pass: ws[0] / ws[1] = max |t| of the force / torque terms (+inf: a non-finite term), ws[2] = 1 if a body id lies outside 0..nbody-1
template <bool BODY>
__global__ void __launch_bounds__(256) k_ibm_force_max(ForceP Q, const double *__restrict__ X, const double *__restrict__ Y, const double *__restrict__ Z, const double *__restrict__ F, const double *__restrict__ dV,
                                                       const int32_t *__restrict__ body, double *__restrict__ ws, unsigned *__restrict__ counter)
{
  __shared__ double red[4][3];
  __shared__ int    flag;
  const int         lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double            m[3] = {0., 0., 0.};
  for (int64_t l = (int64_t)blockIdx.x * 256 + threadIdx.x; l < Q.L; l += (int64_t)gridDim.x * 256) {
    double        t[6];
    const double *ab = Q.about;
    if (BODY) {
      const int b = body[l];
      if (b < 0 || b >= Q.nbody) {
        m[2] = 1.;
        continue;
      }
      ab = ws + FW_ABOUT + 3 * b;
    }
    force_terms(Q, X, Y, Z, F, dV, l, ab, t);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      m[0] = fmax(m[0], force_mag(t[c]));
      m[1] = fmax(m[1], force_mag(t[3 + c]));
    }
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m[a] = fmax(m[a], __shfl_xor(m[a], o, 64));
    if (lane == 0) red[wave][a] = m[a];
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    const double v = fmax(fmax(red[0][threadIdx.x], red[1][threadIdx.x]), fmax(red[2][threadIdx.x], red[3][threadIdx.x]));
    __hip_atomic_store(&ws[FW_PART + 4 * blockIdx.x + threadIdx.x], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if (!force_last_block(counter, &flag)) return;
  if (wave == 0) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      double v = lane < (int)gridDim.x ? __hip_atomic_load(&ws[FW_PART + 4 * lane + a], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
      if (lane == 0) ws[a] = v;
    }
  }
}

// split-and-sum pass: ws[FW_SUMS + (b*6 + term)*2 + part] = the sum over body b's markers of the integers a (part 0) and b (part 1) of term
// 0..2 (force) / 3..5 (torque).  Every partial sum is an exact integer below 2^53, so wave shuffles, LDS atomics and the block order are all free.
template <bool BODY>
__global__ void __launch_bounds__(256) k_ibm_force_sum(ForceP Q, const double *__restrict__ X, const double *__restrict__ Y, const double *__restrict__ Z, const double *__restrict__ F, const double *__restrict__ dV,
                                                       const int32_t *__restrict__ body, double *__restrict__ ws, unsigned *__restrict__ counter)
{
  __shared__ double acc[BODY ? 12 * FORCE_MAXBODY : 4 * 12];
  __shared__ int    flag;
  const int         lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int         n    = 12 * Q.nbody;
  const ForceSplit  sp[2] = {force_split(ws[0]), force_split(ws[1])};
  double            s[12];
#pragma unroll
  for (int j = 0; j < 12; ++j) s[j] = 0.;
  if (BODY) {
    for (int j = threadIdx.x; j < n; j += 256) acc[j] = 0.;
    __syncthreads();
  }
  for (int64_t l = (int64_t)blockIdx.x * 256 + threadIdx.x; l < Q.L; l += (int64_t)gridDim.x * 256) {
    double        t[6];
    const double *ab = Q.about;
    int           b  = 0;
    if (BODY) {
      b = body[l];
      if (b < 0 || b >= Q.nbody) continue;  // the max pass has flagged it: the call fails and the sums are not used
      ab = ws + FW_ABOUT + 3 * b;
    }
    force_terms(Q, X, Y, Z, F, dV, l, ab, t);
#pragma unroll
    for (int c = 0; c < 6; ++c) {
      const ForceSplit &g = sp[c / 3];
      double            ia = 0., ib = 0.;
      if (g.live) {
        ia               = rint(ldexp(t[c], g.sa));
        const double rem = ldexp(t[c], g.up) - ldexp(ia, g.ea);  // exact: the bits of t below 2^(E-30)
        ib               = rint(ldexp(rem, g.sb));
      }
      if (BODY) {
        if (ia != 0.) atomicAdd(&acc[b * 12 + 2 * c], ia);
        if (ib != 0.) atomicAdd(&acc[b * 12 + 2 * c + 1], ib);
      } else {
        s[2 * c] += ia;
        s[2 * c + 1] += ib;
      }
    }
  }
  if (!BODY) {
#pragma unroll
    for (int j = 0; j < 12; ++j) {
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) s[j] += __shfl_xor(s[j], o, 64);
      if (lane == 0) acc[wave * 12 + j] = s[j];
    }
  }
  __syncthreads();
  for (int j = threadIdx.x; j < n; j += 256) {
    const double v = BODY ? acc[j] : (acc[j] + acc[12 + j]) + (acc[24 + j] + acc[36 + j]);
    __hip_atomic_store(&ws[FW_SLAB + (int64_t)blockIdx.x * n + j], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if (!force_last_block(counter, &flag)) return;
  for (int j = threadIdx.x; j < n; j += 256) {
    double v = 0.;
    for (int blk = 0; blk < (int)gridDim.x; ++blk) v += __hip_atomic_load(&ws[FW_SLAB + (int64_t)blk * n + j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    ws[FW_SUMS + j] = v;
  }
}

// ---- Dirichlet forcing of one scalar on the markers (fl_ibm_scalar_force) ---------------------------------------------------------------------
// One pass: Phi = interp(phi), q = T - Phi, Q (+)= q, phi += spread(q, dV) -- the bits of fl_ibm_interp(1), fl_vec_lincomb(-1 Phi + 1 T) and
// fl_ibm_spread(1) one after the other.  The difference is rounded once either way: a product with -1 or 1 is exact.
struct ScalarTarget {
  double value[FORCE_MAXBODY];  // the per-body table, passed by value: the caller's host array is read before the call returns
};
__device__ __forceinline__ double scalar_target(const double *__restrict__ target, const int32_t *__restrict__ body, const ScalarTarget &V, int64_t l)
{
  return target ? target[l] : V.value[body ? body[l] : 0];  // ids are the caller's promise: nothing is clamped or checked here
}

// k_ibm_interp for one field -- its lanes, its weights, its fixed-order reduction -- and lane 0 goes on to the defect: q[l] = T_l - Phi_l,
// Q[l] = q[l] (first pass) or Q[l] + q[l].  One rank only: where partial sums of other ranks belong to Phi, k_ibm_scalar_q forms q behind them.
__global__ void __launch_bounds__(256) k_ibm_scalar_defect(IbmP P, const int *__restrict__ i0, const double *__restrict__ w, const double *__restrict__ phi, const double *__restrict__ target, const int32_t *__restrict__ body,
                                                           ScalarTarget V, int first, double *__restrict__ q, double *__restrict__ Q)
{
  const int     lane = threadIdx.x & 63;
  const int64_t l    = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (l >= P.L) return;
  const int S = P.S;
  const int a = lane % S, b = (lane / S) % S, c3 = lane / (S * S);
  double    wt   = 0.;
  int64_t   cell = -1;
  if (c3 < S) {
    const int ci = support_cell(P, 0, i0[l], a), cj = support_cell(P, 1, i0[P.L + l], b), ck = support_cell(P, 2, i0[2 * P.L + l], c3);
    if (ci >= 0 && cj >= 0 && ck >= 0) {
      cell = ((int64_t)ck * P.n[1] + cj) * P.n[0] + ci;
      wt   = w[(0 * 4 + a) * P.L + l] * w[(1 * 4 + b) * P.L + l] * w[(2 * 4 + c3) * P.L + l];
    }
  }
  double v = cell >= 0 ? wt * phi[cell] : 0.;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  if (lane == 0) {
    const double d = scalar_target(target, body, V, l) - v;
    q[l]           = d;
    if (Q) Q[l] = first ? d : Q[l] + d;
  }
}

// the defect of own marker l from a Phi that is complete (behind k_ibm_collect_U on an owned set, behind the all-reduce on a replicated one)
__global__ void k_ibm_scalar_q(int64_t L, const double *__restrict__ Phi, const double *__restrict__ target, const int32_t *__restrict__ body, ScalarTarget V, int first, double *__restrict__ q, double *__restrict__ Q)
{
  const int64_t l = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (l >= L) return;
  const double d = scalar_target(target, body, V, l) - Phi[l];
  q[l]           = d;
  if (Q) Q[l] = first ? d : Q[l] + d;
}

}  // namespace fl

// ---- force and torque on each body --------------------------------------------------------------------------------------------------------

extern "C" int fl_ibm_force(fl_ibm *m, const double *F, const double *dV, const int32_t *body, int nbody, const double *about, double *force, double *torque)
{
  if (!m) return FL_ERR_ARG_NULL;
  fl_poisson   *h     = m->gp;
  hipStream_t   s     = h->stream;
  const bool    coll  = m->owned && ibm_split(h);  // an owned set on several ranks: collective, every error is voted
  const int64_t L     = m->owned ? m->Lo : m->P.L;
  const bool    null_arg = !force || !about || (L > 0 && (!F || !dV));
  const bool    nbody_ok = nbody >= 1 && nbody <= FORCE_MAXBODY;
  FL_HIP(hipSetDevice(h->device));
  double Lglob = (double)L;
  bool   anybody = body != nullptr;
  if (coll) {
    double v[4] = {null_arg ? 1. : 0., nbody_ok ? 0. : 1., (double)L, body ? 1. : 0.};
    FL_CHK(ibm_vote(h, v, 4));
    if (v[0] > 0.) return FL_ERR_ARG_NULL;
    if (v[1] > 0.) return FL_ERR_ARG_OUTOFRANGE;
    Lglob   = v[2];
    anybody = v[3] > 0.;  // a rank without markers may leave the body array out: every rank still reduces the same number of sums
  } else {
    if (null_arg) return FL_ERR_ARG_NULL;
    if (!nbody_ok) return FL_ERR_ARG_OUTOFRANGE;
  }
  if (Lglob >= (double)((int64_t)1 << 22)) return FL_ERR_SUP;  // beyond it the integer sums could leave the 53 bits of a double
  const int nbk = body ? nbody : 1;     // bodies the kernels index on this rank
  const int nb  = anybody ? nbody : 1;  // bodies the sums are kept for
  const int n   = 12 * nb;
  std::vector<double> host((size_t)(FW_SUMS + n), 0.);
  if (L > 0) {
    if (m->fws.once(h, FW_END, true)) return FL_ERR_MEM;
    if (m->ftick.once(h, 4, true)) return FL_ERR_MEM;
  }
  ForceP Q;
  Q.L     = L;
  Q.nbody = nbk;
  for (int d = 0; d < 3; ++d) {
    const Axis &A  = h->ax[d];
    Q.periodic[d] = A.periodic ? 1 : 0;
    Q.per[d]      = A.xf[A.n] - A.xf[0];
    Q.about[d]    = about[d];
  }
  const int nblk = (int)std::min<int64_t>((L + 255) / 256, FORCE_MAXBLK);
  if (L > 0) {
    FL_HIP(hipMemsetAsync(m->ftick, 0, 16, s));
    if (body) FL_HIP(hipMemcpyAsync(m->fws + FW_ABOUT, about, sizeof(double) * 3 * (size_t)nbk, hipMemcpyHostToDevice, s));
    if (body) hipLaunchKernelGGL(k_ibm_force_max<true>, dim3(nblk), dim3(256), 0, s, Q, m->X, m->Y, m->Z, F, dV, body, m->fws, m->ftick);
    else hipLaunchKernelGGL(k_ibm_force_max<false>, dim3(nblk), dim3(256), 0, s, Q, m->X, m->Y, m->Z, F, dV, body, m->fws, m->ftick);
    FL_HIP(hipGetLastError());
  }
  if (coll) {
    // the two maxima and the flag over the ranks, then back to the device: every rank splits by the same E
    if (L > 0) {
      FL_HIP(hipMemcpyAsync(host.data(), m->fws, sizeof(double) * 4, hipMemcpyDeviceToHost, s));
      FL_HIP(hipStreamSynchronize(s));
    }
    FL_CHK(fl_allreduce_max(h, &host[0]));
    FL_CHK(fl_allreduce_max(h, &host[1]));
    FL_CHK(ibm_vote(h, &host[2], 1));
    if (host[2] > 0.) return FL_ERR_ARG_OUTOFRANGE;
    if (L > 0) FL_HIP(hipMemcpyAsync(m->fws, host.data(), sizeof(double) * 2, hipMemcpyHostToDevice, s));
  }
  if (L > 0) {
    if (body) hipLaunchKernelGGL(k_ibm_force_sum<true>, dim3(nblk), dim3(256), 0, s, Q, m->X, m->Y, m->Z, F, dV, body, m->fws, m->ftick + 1);
    else hipLaunchKernelGGL(k_ibm_force_sum<false>, dim3(nblk), dim3(256), 0, s, Q, m->X, m->Y, m->Z, F, dV, body, m->fws, m->ftick + 1);
    FL_HIP(hipGetLastError());
    const double amax[2] = {host[0], host[1]};
    FL_HIP(hipMemcpyAsync(host.data(), m->fws, sizeof(double) * (size_t)(FW_SUMS + 12 * nbk), hipMemcpyDeviceToHost, s));
    FL_HIP(hipStreamSynchronize(s));  // the one host wait of a call on one rank
    if (coll) host[0] = amax[0], host[1] = amax[1];
    else if (host[2] > 0.) return FL_ERR_ARG_OUTOFRANGE;
  }
  if (coll)  // sums of exact integers stay exact: eight at a time through the handle's sum all-reduce
    for (int j = 0; j < n; j += 8) FL_CHK(fl_poisson_allreduce_sum(h, &host[(size_t)(FW_SUMS + j)], std::min(8, n - j)));
  for (int b = 0; b < nbody; ++b)
    for (int c = 0; c < 3; ++c) {
      const double *q = &host[(size_t)(FW_SUMS + 12 * (b < nb ? b : 0))];
      force[3 * b + c] = b < nb ? force_combine(host[0], q[2 * c], q[2 * c + 1]) : (host[0] <= 1.7976931348623157e308 ? 0. : std::nan(""));
      if (torque) torque[3 * b + c] = b < nb ? force_combine(host[1], q[2 * (3 + c)], q[2 * (3 + c) + 1]) : (host[1] <= 1.7976931348623157e308 ? 0. : std::nan(""));
    }
  return FL_SUCCESS;
}

// ---- Dirichlet forcing of one scalar, and what it hands to the fluid ------------------------------------------------------------------------

extern "C" int fl_ibm_scalar_force(fl_ibm *m, int npass, const double *target_dev, const int32_t *body_dev, int nbody, const double *value, const double *dV_dev, double *phi_dev, double *Q_dev)
{
  if (!m) return FL_ERR_ARG_NULL;
  fl_poisson   *h     = m->gp;
  hipStream_t   s     = h->stream;
  const bool    split = h->multi || ibm_split(h);
  const int64_t L     = m->owned ? m->Lo : m->P.L;
  const bool    null_arg = !phi_dev || (L > 0 && !dV_dev);
  const bool    range_ok = npass >= 1 && npass <= 16 && nbody >= 1 && nbody <= FORCE_MAXBODY;
  const bool    wrong    = (target_dev && value) || (L > 0 && !target_dev && !value);
  FL_HIP(hipSetDevice(h->device));
  if (m->owned && split) {  // collective: every rank leaves with the same error, or none does
    double v[3] = {null_arg ? 1. : 0., range_ok ? 0. : 1., wrong ? 1. : 0.};
    FL_CHK(ibm_vote(h, v, 3));
    if (v[0] > 0.) return FL_ERR_ARG_NULL;
    if (v[1] > 0.) return FL_ERR_ARG_OUTOFRANGE;
    if (v[2] > 0.) return FL_ERR_ARG_WRONG;
  } else {
    if (null_arg) return FL_ERR_ARG_NULL;
    if (!range_ok) return FL_ERR_ARG_OUTOFRANGE;
    if (wrong) return FL_ERR_ARG_WRONG;
  }
  ScalarTarget V;
  for (int b = 0; b < FORCE_MAXBODY; ++b) V.value[b] = (value && b < nbody) ? value[b] : 0.;
  const int32_t *body = value ? body_dev : nullptr;
  if (L > 0) FL_CHK(m->sq.reserve(h, L));
  if (L > 0 && split) FL_CHK(m->sphi.reserve(h, L));
  const unsigned nbq = (unsigned)((L + 255) / 256);
  for (int k = 0; k < npass; ++k) {
    if (!split) {
      // one rank: every marker's support is here (P.L = L, an owned set holds no ghost) -- the defect in the interpolation's launch
      if (L > 0) hipLaunchKernelGGL(k_ibm_scalar_defect, dim3((unsigned)((L + 3) / 4)), dim3(256), 0, s, m->P, m->i0, m->w, phi_dev, target_dev, body, V, k == 0, m->sq, Q_dev);
      ibm_launch_spread(m, 1, m->sq, dV_dev, phi_dev, true);
      FL_HIP(hipGetLastError());
    } else if (m->owned) {
      FL_CHK(ibm_interp_owned(m, 1, phi_dev, m->sphi));  // own + ghost markers, the ghosts' partial sums back to their owners
      if (L > 0) hipLaunchKernelGGL(k_ibm_scalar_q, dim3(nbq), dim3(256), 0, s, L, m->sphi, target_dev, body, V, k == 0, m->sq, Q_dev);
      FL_HIP(hipGetLastError());
      FL_CHK(ibm_spread_owned(m, 1, m->sq, dV_dev, phi_dev, true));
    } else {
      ibm_launch_interp(m, L, 1, phi_dev, m->sphi);
      FL_HIP(hipGetLastError());
      if (h->comm.kind == Comm::NONE) return FL_ERR_ARG_WRONGSTATE;
      FL_CHK(h->comm.allreduce(s, m->sphi, (int)L));  // where fl_ibm_interp has it
      hipLaunchKernelGGL(k_ibm_scalar_q, dim3(nbq), dim3(256), 0, s, L, m->sphi, target_dev, body, V, k == 0, m->sq, Q_dev);
      ibm_launch_spread(m, 1, m->sq, dV_dev, phi_dev, true);
      FL_HIP(hipGetLastError());
    }
  }
  return FL_SUCCESS;
}

// The sum is fl_ibm_force's, on F = (Q, 0, 0): its force group then holds the terms Q_l dV_l and nothing else (a zero term changes neither the
// maximum nor an integer sum), so the split, the bound, the NaN rule, the votes and the collectives are that call's own.  The torque group it
// also forms is not used.
extern "C" int fl_ibm_scalar_rate(fl_ibm *m, const double *Q_dev, const double *dV_dev, const int32_t *body_dev, int nbody, double *rate)
{
  if (!m) return FL_ERR_ARG_NULL;
  fl_poisson   *h = m->gp;
  const int64_t L = m->owned ? m->Lo : m->P.L;
  FL_HIP(hipSetDevice(h->device));
  const double *F = nullptr;
  if (L > 0 && Q_dev) {
    FL_CHK(m->sf3.reserve(h, 3 * L));
    FL_HIP(hipMemcpyAsync(m->sf3, Q_dev, sizeof(double) * (size_t)L, hipMemcpyDeviceToDevice, h->stream));
    FL_HIP(hipMemsetAsync(m->sf3 + L, 0, sizeof(double) * 2 * (size_t)L, h->stream));
    F = m->sf3;
  }
  const int           nb = std::min(std::max(nbody, 1), FORCE_MAXBODY);
  std::vector<double> about(3 * (size_t)nb, 0.), force(3 * (size_t)nb, 0.);
  // nbody out of range: fl_ibm_force says so (and votes it) before it reads or writes an array sized by it
  const int rc = fl_ibm_force(m, F, dV_dev, body_dev, nbody, about.data(), rate ? force.data() : nullptr, nullptr);
  if (rc) return rc;
  for (int b = 0; b < nbody; ++b) rate[b] = force[3 * (size_t)b];
  return FL_SUCCESS;
}
