// fl_abf.hip -- the ABF block preconditioner around the momentum operator of fl_momentum.hip: the cell-to-face interpolations T and B, MatMult of the
// 3 x 3 Jacobian the preconditioner is built for, the DIAG / ROWSUM Schur product with its flexible GMRES, and PCApply_ABF (abfpc.c:48-111).
#include "fl_gmres_lsq.h"
#include "fl_mom_handle.h"

namespace fl {

// out = 1 / in   (VecReciprocal)
__global__ void __launch_bounds__(256) k_recip(int64_t n, const double *__restrict__ in, double *__restrict__ out)
{
  for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < n; q += (int64_t)gridDim.x * blockDim.x) out[q] = 1. / in[q];
}
// y = (w - shift) .* x  [+ y]   (VecPointwiseMult with the scaling 1/a or 1/a - 1)
__global__ void __launch_bounds__(256) k_scale_by(int64_t n, const double *__restrict__ w, double shift, const double *x, double *y, int add)
{
  for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < n; q += (int64_t)gridDim.x * blockDim.x) {
    const double t = (w[q] - shift) * x[q];
    y[q]           = add ? y[q] + t : t;
  }
}

// V_d = rhs_d + alpha (T v)_d on the owned d-faces (unpadded face array, rhs may alias V); v: padded component d with valid ghosts
__global__ void __launch_bounds__(256) k_face_interp(GridP g, FaceT t, int kind, int d, double alpha, const double *__restrict__ vpad, const double *rhs, double *V)
{
  // a wave per 64-face row segment: row and plane numbers are wave-uniform (scalar index arithmetic and, for d != 0, scalar table reads)
  const int     ex = d == 0 ? g.fx : g.nx, ey = d == 1 ? g.fy : g.ny, ez = d == 2 ? g.fz : g.nz;
  const int64_t str = d == 0 ? 1 : (d == 1 ? (int64_t)g.sx : g.sxy);
  const int     lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), nw = blockDim.x >> 6;
  const int     nseg = (ex + 63) / 64;
  const int64_t nitem = (int64_t)nseg * ey * ez;
  for (int64_t it = (int64_t)blockIdx.x * nw + w; it < nitem; it += (int64_t)gridDim.x * nw) {
    const int seg = (int)(it % nseg), row = (int)(it / nseg);
    const int j = row % ey, k = row / ey, i = seg * 64 + lane;
    if (i >= ex) continue;
    const int     f = d == 0 ? i : (d == 1 ? j : k);
    const int     c0 = t.c0[kind][d][f];
    const int64_t q = ((int64_t)k * ey + j) * ex + i;
    // cell (i,j,k) with the d-th index replaced by c0
    const int64_t base = g.off0 + (int64_t)k * g.sxy + (int64_t)j * g.sx + i + (int64_t)(c0 - f) * str;
    const double  w0 = alpha * t.w0[kind][d][f], w1 = alpha * t.w1[kind][d][f];
    double        s = rhs ? rhs[q] : 0.;
    if (w0 != 0.) s += w0 * vpad[base];
    if (w1 != 0.) s += w1 * vpad[base + str];
    V[q] = s;
  }
}

// The same row on the faces at the two ends of axis d only (face 0 and, where this rank owns it, face n_d): all fl_momentum_set_state_v0 reads of a
// stored v0interp field.  One thread per face of the two planes.
__global__ void __launch_bounds__(256) k_face_interp_ends(GridP g, FaceT t, int kind, int d, const double *__restrict__ vpad, const double *rhs, double *V)
{
  const int     ex = d == 0 ? g.fx : g.nx, ey = d == 1 ? g.fy : g.ny, ez = d == 2 ? g.fz : g.nz;
  const int     nd = d == 0 ? g.nx : (d == 1 ? g.ny : g.nz), ed = d == 0 ? ex : (d == 1 ? ey : ez);
  const int     na = d == 0 ? ey : ex, nb = d == 2 ? ey : ez;
  const int64_t n = (int64_t)na * nb * (ed > nd ? 2 : 1);
  const int64_t str = d == 0 ? 1 : (d == 1 ? (int64_t)g.sx : g.sxy);
  for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < n; q += (int64_t)gridDim.x * blockDim.x) {
    const int     a = (int)(q % na), b = (int)((q / na) % nb), f = (q / ((int64_t)na * nb)) ? nd : 0;
    const int     i = d == 0 ? f : a, j = d == 1 ? f : (d == 0 ? a : b), k = d == 2 ? f : b;
    const int64_t u = ((int64_t)k * ey + j) * ex + i;
    const int     c0 = t.c0[kind][d][f];
    const int64_t base = g.off0 + (int64_t)k * g.sxy + (int64_t)j * g.sx + i + (int64_t)(c0 - f) * str;
    const double  w0 = t.w0[kind][d][f], w1 = t.w1[kind][d][f];
    double        s = rhs ? rhs[u] : 0.;
    if (w0 != 0.) s += w0 * vpad[base];
    if (w1 != 0.) s += w1 * vpad[base + str];
    V[u] = s;
  }
}

}  // namespace fl

using namespace fl;

namespace {

int face_interp(fl_momentum *m, double alpha, const double *v_dev, const double *const rhs_dev[3], double *const V_dev[3])
{
  fl_poisson *h = m->p;
  FL_CHK(mom_stage(m, v_dev));
  for (int d = 0; d < 3; ++d) {
    if (!V_dev[d]) return FL_ERR_ARG_NULL;
    hipLaunchKernelGGL(k_face_interp, dim3(nblk_flat(h->nface[d])), dim3(256), 0, h->stream, h->g, m->ft, 0, d, alpha, m->vec[7] + (size_t)d * h->padlen, rhs_dev ? rhs_dev[d] : nullptr, V_dev[d]);
  }
  FL_HIP(hipGetLastError());
  return 0;
}

}  // namespace

// V* = interprhs - (-T) v*   (MatMult(negT) + VecAYPX, abfpc.c:73-74)
extern "C" int fl_momentum_face_interp(fl_momentum *m, const double *v_dev, const double *const rhs_dev[3], double *const V_dev[3])
{
  if (!m || !v_dev || !V_dev) return FL_ERR_ARG_NULL;
  FL_HIP(hipSetDevice(m->p->device));
  return face_interp(m, 1., v_dev, rhs_dev, V_dev);
}

extern "C" int fl_momentum_face_interp_scaled(fl_momentum *m, double alpha, const double *v_dev, const double *const rhs_dev[3], double *const V_dev[3])
{
  if (!m || !v_dev || !V_dev) return FL_ERR_ARG_NULL;
  FL_HIP(hipSetDevice(m->p->device));
  return face_interp(m, alpha, v_dev, rhs_dev, V_dev);
}

// v0interp = B v0 (+ vbc): MatMult(cnl->B, v0, cnl->v0interp); VecAXPY(v0interp, 1, vbc), cnlinearcart3d.c:2826-2829
extern "C" int fl_momentum_interp_faces(fl_momentum *m, const double *v_dev, const double *const vbc_dev[9], double *const out_dev[9])
{
  if (!m || !v_dev || !out_dev) return FL_ERR_ARG_NULL;
  fl_poisson *h = m->p;
  FL_HIP(hipSetDevice(h->device));
  FL_CHK(mom_stage(m, v_dev));
  for (int c = 0; c < 3; ++c)
    for (int d = 0; d < 3; ++d) {
      if (!out_dev[c * 3 + d]) return FL_ERR_ARG_NULL;
      hipLaunchKernelGGL(k_face_interp, dim3(nblk_flat(h->nface[d])), dim3(256), 0, h->stream, h->g, m->ft, c == d ? 1 : 2, d, 1., m->vec[7] + (size_t)c * h->padlen, vbc_dev ? vbc_dev[c * 3 + d] : nullptr,
                         out_dev[c * 3 + d]);
    }
  FL_HIP(hipGetLastError());
  return FL_SUCCESS;
}

// The block-end faces of the same nine fields only (face 0 and face n of each axis, where this rank owns them): what fl_momentum_set_state_v0 reads of
// v0interp when the operator forms the inner faces from v0 itself.  The inner entries of out_dev are NOT written.
extern "C" int fl_momentum_interp_faces_ends(fl_momentum *m, const double *v_dev, const double *const vbc_dev[9], double *const out_dev[9])
{
  if (!m || !v_dev || !out_dev) return FL_ERR_ARG_NULL;
  fl_poisson *h = m->p;
  const GridP &g = h->g;
  // where the operator will read whole fields (k_mom2: a block with ny <= 8) the whole fields are what is needed
  if (!mom3_grid(g)) return fl_momentum_interp_faces(m, v_dev, vbc_dev, out_dev);
  FL_HIP(hipSetDevice(h->device));
  FL_CHK(mom_stage(m, v_dev));
  for (int c = 0; c < 3; ++c)
    for (int d = 0; d < 3; ++d) {
      if (!out_dev[c * 3 + d]) return FL_ERR_ARG_NULL;
      const int64_t n = 2 * h->nface[d] / std::max(d == 0 ? g.fx : (d == 1 ? g.fy : g.fz), 1);
      hipLaunchKernelGGL(k_face_interp_ends, dim3(nblk_flat(n)), dim3(256), 0, h->stream, g, m->ft, c == d ? 1 : 2, d, m->vec[7] + (size_t)c * h->padlen, vbc_dev ? vbc_dev[c * 3 + d] : nullptr, out_dev[c * 3 + d]);
    }
  FL_HIP(hipGetLastError());
  return FL_SUCCESS;
}

// MatMult(J) of the 3 x 3 MatNest the preconditioner is built for (NSFormJacobian_CNLinear_Cart3d_Internal,
// cnlinearcart3d.c:2885-2941):  rows v: [A, 0, kappa G]   V: [-T, I, -R]   p: [0, D, 0],   -R = (-T)(kappa G) + kappa Gst
extern "C" int fl_abf_jacobian_mult(fl_momentum *m, const double *v_dev, const double *const V_dev[3], const double *p_dev, double *fv_dev, double *const fV_dev[3], double *fp_dev)
{
  if (!m || !v_dev || !V_dev || !p_dev || !fv_dev || !fV_dev || !fp_dev) return FL_ERR_ARG_NULL;
  fl_poisson *h = m->p;
  FL_HIP(hipSetDevice(h->device));
  const int64_t N = h->ncell;
  FL_CHK(m->tmpv.once(h, 3 * N, true));
  FL_CHK(m->srhs.once(h, N, true));
  for (int d = 0; d < 3; ++d)
    if (!V_dev[d] || !fV_dev[d]) return FL_ERR_ARG_NULL;
  FL_CHK(fl_momentum_apply(m, v_dev, fv_dev));                                                        // fv = A v
  lincomb(h, N, -1., p_dev, 0., nullptr, m->srhs);                                                    // -p
  lincomb(h, 3 * N, 1., v_dev, 0., nullptr, m->tmpv);                                                 // w = v
  for (int d = 0; d < 3; ++d) lincomb(h, h->nface[d], 1., V_dev[d], 0., nullptr, fV_dev[d]);          // fV = V
  FL_CHK(fl_poisson_project(h, m->srhs, m->tmpv, m->tmpv + N, m->tmpv + 2 * N, fV_dev[0], fV_dev[1], fV_dev[2]));  // w = v + kappa G p ; fV = V + kappa Gst p
  lincomb(h, 3 * N, 1., fv_dev, 1., m->tmpv, fv_dev);                                                 // fv += w
  lincomb(h, 3 * N, 1., fv_dev, -1., v_dev, fv_dev);                                                  // fv -= v      -> A v + kappa G p
  FL_CHK(face_interp(m, -1., m->tmpv, fV_dev, fV_dev));                                               // fV -= T w    -> V - T v - T kappa G p + kappa Gst p
  FL_CHK(fl_poisson_rhs(h, V_dev[0], V_dev[1], V_dev[2], nullptr, fp_dev));                           // -D V
  lincomb(h, N, -1., fp_dev, 0., nullptr, fp_dev);                                                    // fp = D V
  FL_HIP(hipGetLastError());
  return FL_SUCCESS;
}

// ------------------------------------------------------------------------------------------------ schurainv / upperainv
// PC_ABF_AINV_DIAG / ROWSUM (abfpc.c:81-94, 151-171).  With a = diag(A) or A 1 and -R = (-T)(kappa G) + kappa Gst:
//   S     = D ((-T) a^-1 kappa G - (-R)) = -D [ T ((a^-1 - 1) .* kappa G p) + kappa Gst p ]          (schurainv)
//   stage 2: v = v* - a^-1 .* kappa G p ;  V = V* - T ((a^-1 - 1) .* kappa G p) - kappa Gst p          (upperainv)
// S is then a variable-coefficient 13-point operator that changes every step.  It is applied as the composition of the
// kernels that exist (cell gradient + staggered gradient, scaling, face interpolation, divergence) and solved by flexible
// GMRES preconditioned with the constant-coefficient Schur solve (the ID operator: a = 1 + O(dt) keeps S close to it).  This is
// the non-default option of the reference; the fused matrix-free path is the ID one.
namespace {

// out (3 * cells, unpadded) = 1 / diag(A)  or  1 / (A 1)
int compute_ainv(fl_momentum *m, int type, DevBuf<double> &out)
{
  fl_poisson   *h = m->p;
  const int64_t n3 = 3 * h->ncell;
  FL_CHK(out.once(h, n3, true));
  if (type == FL_ABF_AINV_DIAG) FL_CHK(fl_momentum_diagonal(m, out));  // MatGetDiagonal(A)
  else FL_CHK(fl_momentum_rowsum(m, out));                             // MatGetRowSum(A)
  hipLaunchKernelGGL(k_recip, dim3(nblk_flat(n3)), dim3(256), 0, h->stream, n3, (const double *)out, out.p);  // VecReciprocal
  return 0;
}

int ensure_ainv_scratch(fl_momentum *m)
{
  fl_poisson *h = m->p;
  FL_CHK(m->gv.once(h, 3 * h->ncell, true));
  for (int d = 0; d < 3; ++d) FL_CHK(m->zV[d].once(h, std::max<int64_t>(h->nface[d], 1), true));
  return 0;
}

// y = S p with S = D ((-T) a^-1 kappa G - (-R)), a^-1 in m->ainv[0]
int schur_apply_var(fl_momentum *m, const double *p, double *y)
{
  fl_poisson   *h = m->p;
  const int64_t N = h->ncell, n3 = 3 * N;
  if (knob(K_schur_var_fused) != 0 && fl_schur_var_usable(h)) {  // one pass over p and a^-1 (fl_schur_var.hip), on one rank or several
    FL_CHK(fl_ensure_vec(h, &h->w0));
    launch_pad_copy(h->stream, h->g, p, h->w0);
    FL_CHK(fl_schur_var_fill_ghosts(h, h->w0));
    SchurVarT t;
    for (int d = 0; d < 3; ++d) {
      t.w0[d] = m->ft.w0[0][d];
      t.w1[d] = m->ft.w1[0][d];
      t.c0[d] = m->ft.c0[0][d];
    }
    return fl_schur_var_apply_fused(h, t, m->ainv[0], h->w0, y);
  }
  FL_CHK(ensure_ainv_scratch(m));
  double *const zV[3] = {m->zV[0], m->zV[1], m->zV[2]};
  FL_HIP(hipMemsetAsync(m->gv, 0, sizeof(double) * (size_t)n3, h->stream));
  for (int d = 0; d < 3; ++d) FL_HIP(hipMemsetAsync(zV[d], 0, sizeof(double) * (size_t)h->nface[d], h->stream));
  FL_CHK(fl_poisson_project(h, p, m->gv, m->gv + N, m->gv + 2 * N, zV[0], zV[1], zV[2]));                 // gv = -kappa G p ; zV = -kappa Gst p
  hipLaunchKernelGGL(k_scale_by, dim3(nblk_flat(n3)), dim3(256), 0, h->stream, n3, (const double *)m->ainv[0], 1., (const double *)m->gv, m->gv.p, 0);  // gv *= a^-1 - 1
  FL_CHK(face_interp(m, 1., m->gv, zV, zV));                                                              // zV += T gv
  FL_CHK(fl_poisson_rhs(h, zV[0], zV[1], zV[2], nullptr, y));                                             // y = -D zV
  lincomb(h, N, -1., y, 0., nullptr, y);                                                                  // y = D zV = S p
  return 0;
}

// KSPSolve(kspS) for the variable-coefficient S: flexible GMRES(20), right preconditioner = the constant-coefficient Schur solve
// with the caller's options (its tolerance loosened to 1e-2: the outer iteration is flexible).  Unpreconditioned residual
// norm against opts->rtol / atol, zero initial guess.
int schur_solve_var(fl_momentum *m, const double *b, double *x, const fl_ksp_opts *o, fl_ksp_stats *st)
{
  fl_poisson   *h = m->p;
  const int64_t N = h->ncell;
  constexpr int M = 20;
  // vectors: V_0..V_M, Z_0..Z_{M-1}, w
  while ((int)m->gm.size() < 2 * M + 2) {
    DevBuf<double> v;
    FL_CHK(v.exact(h, N, true));
    m->gm.push_back(std::move(v));
  }
  DevBuf<double> *V = m->gm.data(), *Z = m->gm.data() + M + 1;
  double         *w = m->gm[2 * M + 1];
  fl_ksp_opts inner = *o;
  inner.rtol        = std::max(o->rtol, 1e-2);
  inner.history     = nullptr;
  inner.nhistory    = 0;
  fl_ksp_stats ist;
  struct Events {  // released on every return path
    hipEvent_t a = nullptr, b = nullptr;
    ~Events()
    {
      if (a) (void)hipEventDestroy(a);
      if (b) (void)hipEventDestroy(b);
    }
  } ev;
  FL_HIP(hipEventCreate(&ev.a));
  FL_HIP(hipEventCreate(&ev.b));
  hipEvent_t e0 = ev.a, e1 = ev.b;
  FL_HIP(hipEventRecord(e0, h->stream));
  GmresLsq lsq(M);
  double   hcol[M + 1], y[M];
  double   bnorm = 0., beta = 0.;
  FL_CHK(fl_vec_dot(h, N, b, b, &bnorm));
  bnorm = std::sqrt(bnorm);
  const double ttol = std::max(o->rtol * bnorm, o->atol);
  FL_HIP(hipMemsetAsync(x, 0, sizeof(double) * (size_t)N, h->stream));
  int    its = 0, reason = 0, nh = 0;
  double rnorm = bnorm;
  if (o->history && o->nhistory > 0) o->history[nh++] = bnorm;
  bool first = true;
  while (!reason) {
    if (first) lincomb(h, N, 1., b, 0., nullptr, w);
    else {
      FL_CHK(schur_apply_var(m, x, w));
      lincomb(h, N, -1., w, 1., b, w);  // r = b - S x
    }
    first = false;
    FL_CHK(fl_vec_dot(h, N, w, w, &beta));
    beta  = std::sqrt(beta);
    rnorm = beta;
    if (std::isnan(beta)) { reason = FL_DIVERGED_NANORINF; break; }
    if (beta <= ttol) { reason = beta < o->atol ? FL_CONVERGED_ATOL : FL_CONVERGED_RTOL; break; }
    if (its >= o->maxit) { reason = FL_DIVERGED_ITS; break; }
    lincomb(h, N, 1. / beta, w, 0., nullptr, V[0]);
    lsq.reset(beta);
    int j = 0;
    for (; j < M && its < o->maxit; ++j) {
      FL_CHK(fl_poisson_solve(h, V[j], Z[j], &inner, &ist));  // z_j = S_ID^-1 v_j
      if (ist.reason < 0 && ist.reason != FL_DIVERGED_ITS) { reason = ist.reason; break; }
      FL_CHK(schur_apply_var(m, Z[j], w));                    // w = S z_j
      for (int i = 0; i <= j; ++i) {                          // modified Gram-Schmidt
        FL_CHK(fl_vec_dot(h, N, w, V[i], &hcol[i]));
        lincomb(h, N, 1., w, -hcol[i], V[i], w);
      }
      double hn;
      FL_CHK(fl_vec_dot(h, N, w, w, &hn));
      hn = std::sqrt(hn);
      hcol[j + 1] = hn;
      rnorm = lsq.push(j, hcol);
      ++its;
      if (o->history && nh < o->nhistory) o->history[nh++] = rnorm;
      if (rnorm <= ttol || hn == 0.) {
        ++j;
        break;
      }
      lincomb(h, N, 1. / hn, w, 0., nullptr, V[j + 1]);
    }
    lsq.solve(j, y);  // y = H^-1 g ; x += Z y
    for (int i = 0; i < j; ++i) lincomb(h, N, 1., x, y[i], Z[i], x);
    if (reason) break;
  }
  FL_HIP(hipEventRecord(e1, h->stream));
  FL_HIP(hipStreamSynchronize(h->stream));
  float ms = 0.f;
  FL_HIP(hipEventElapsedTime(&ms, e0, e1));
  st->iters   = its;
  st->reason  = reason;
  st->rnorm0  = bnorm;
  st->rnorm   = rnorm;
  st->seconds = ms * 1e-3;
  return 0;
}

}  // namespace

extern "C" int fl_abf_set_ainv_types(fl_momentum *m, int schur_type, int upper_type)
{
  if (!m) return FL_ERR_ARG_NULL;
  for (int t : {schur_type, upper_type})
    if (t != FL_ABF_AINV_ID && t != FL_ABF_AINV_DIAG && t != FL_ABF_AINV_ROWSUM) return FL_ERR_SUP;  // "Unsupported Ainv type"
  m->schur_ainv = schur_type;
  m->upper_ainv = upper_type;
  return FL_SUCCESS;
}

extern "C" int fl_abf_schur_apply(fl_momentum *m, const double *p_dev, double *y_dev)
{
  if (!m || !p_dev || !y_dev) return FL_ERR_ARG_NULL;
  fl_poisson *h = m->p;
  FL_HIP(hipSetDevice(h->device));
  if (m->schur_ainv == FL_ABF_AINV_ID) return fl_poisson_apply(h, p_dev, y_dev);
  if (!m->have_state && m->mp.cC != 0.) return FL_ERR_ARG_WRONGSTATE;
  FL_CHK(compute_ainv(m, m->schur_ainv, m->ainv[0]));
  FL_CHK(schur_apply_var(m, p_dev, y_dev));
  FL_HIP(hipGetLastError());
  return FL_SUCCESS;
}

// PCApply_ABF (abfpc.c:48-111), start to finish on the device; schurainv / upperainv as set by fl_abf_set_ainv_types (default ID)
extern "C" int fl_abf_apply(fl_momentum *m, const fl_ksp_opts *momentum_opts, const fl_ksp_opts *schur_opts, const double *momrhs_dev, const double *const interprhs_dev[3], const double *contrhs_dev,
                            double *v_dev, double *const V_dev[3], double *p_dev, fl_ksp_stats stats[2])
{
  if (!m || !momentum_opts || !schur_opts || !momrhs_dev || !v_dev || !V_dev || !p_dev || !stats) return FL_ERR_ARG_NULL;
  fl_poisson *h = m->p;
  FL_HIP(hipSetDevice(h->device));
  FL_CHK(m->srhs.once(h, h->ncell, true));
  /* stage 1: the lower-triangular factor */
  FL_CHK(fl_momentum_solve(m, momrhs_dev, v_dev, momentum_opts, &stats[0]));                        /* :72     v* = A^-1 momrhs */
  FL_CHK(fl_momentum_face_interp(m, v_dev, interprhs_dev, V_dev));                                  /* :73-74  V* = interprhs + T v* */
  FL_CHK(fl_poisson_rhs(h, V_dev[0], V_dev[1], V_dev[2], contrhs_dev, m->srhs));                    /* :75-76  Srhs = contrhs - D V* */
  const size_t N = (size_t)h->ncell;
  if (m->schur_ainv == FL_ABF_AINV_ID) FL_CHK(fl_poisson_solve(h, m->srhs, p_dev, schur_opts, &stats[1]));   /* :77     p = S^-1 Srhs */
  else {
    FL_CHK(compute_ainv(m, m->schur_ainv, m->ainv[0]));                                             /* :155-165 (PCSetUp: S follows A) */
    FL_CHK(schur_solve_var(m, m->srhs, p_dev, schur_opts, &stats[1]));
  }
  /* stage 2: the upper-triangular factor; with upperainv = ID, (-T)(Gp) - (-R)p == -kappa Gst p, see DESIGN.md section 1 */
  if (m->upper_ainv == FL_ABF_AINV_ID) return fl_poisson_project(h, p_dev, v_dev, v_dev + N, v_dev + 2 * N, V_dev[0], V_dev[1], V_dev[2]);   /* :80-101 */
  FL_CHK(compute_ainv(m, m->upper_ainv, m->ainv[1]));                                               /* :84-90 */
  FL_CHK(ensure_ainv_scratch(m));
  const int64_t n3 = 3 * (int64_t)N;
  FL_HIP(hipMemsetAsync(m->gv, 0, sizeof(double) * (size_t)n3, h->stream));
  FL_CHK(fl_poisson_project(h, p_dev, m->gv, m->gv + N, m->gv + 2 * N, V_dev[0], V_dev[1], V_dev[2]));     /* gv = -kappa G p ; V = V* - kappa Gst p */
  hipLaunchKernelGGL(k_scale_by, dim3(nblk_flat(n3)), dim3(256), 0, h->stream, n3, (const double *)m->ainv[1], 0., (const double *)m->gv, v_dev, 1);   /* v = v* - a^-1 kappa G p  (:91,95) */
  hipLaunchKernelGGL(k_scale_by, dim3(nblk_flat(n3)), dim3(256), 0, h->stream, n3, (const double *)m->ainv[1], 1., (const double *)m->gv, m->gv.p, 0);  /* gv = -(a^-1 - 1) kappa G p */
  FL_CHK(face_interp(m, 1., m->gv, V_dev, V_dev));                                                  /* V -= T ((a^-1 - 1) kappa G p)  (:96-101) */
  FL_HIP(hipGetLastError());
  return FL_SUCCESS;
}
