// fl_mom_handle.h -- the fl_momentum handle, the two structs its kernels take, and the host functions that cross between fl_momentum.hip (the
// operator), fl_mom_solve.hip (the Krylov drivers on it), fl_abf.hip (face interpolation, the block preconditioner) and fl_vec.hip (BLAS-1 on device
// vectors).  Every __global__ function lives in exactly one of the four; a unit that needs another's kernel calls one of the launchers declared below.
#pragma once
#include <vector>

#include "fl_devbuf.h"
#include "fl_handle.h"

namespace fl {

struct MomP {
  const double *tab[3];   // MOM_NTAB x len, slot-major, LOCAL block of each axis
  const double *stab[3];  // the same numbers times (cC, cL), cell-major (k_mom_scale_tab): what k_mom2 reads
  const double *bw[3];    // rows of B (build_axis_faceinterp) per LOCAL face, face-major: w0, w1 of the normal rule, w0, w1 of the tangential rule (k_mom3)
  int           len[3];
  double        cI, cC, cL;
};

// cell-to-face interpolation rows (build_axis_faceinterp): per LOCAL face of each axis, V_f = w0 v[c0] + w1 v[c0 + 1]
// (c0 local, -1 = low ghost).  kind 0 = T, 1 = B normal component, 2 = B tangential component.
struct FaceT {
  const double *w0[3][3], *w1[3][3];  // [kind][axis]
  const int    *c0[3][3];
};

}  // namespace fl

#pragma GCC visibility push(hidden)  // internal to the library: its dynamic symbols stay the C-ABI's

// Device arrays the handle owns are DevBufs (freed with the handle, in the order of the members); what it borrows is a plain pointer: p, the views in
// mp / ft.
struct fl_momentum {
  fl_poisson *p = nullptr;
  fl::MomP    mp;
  fl::FaceT   ft;
  fl::DevBuf<double> tabs[3];
  fl::DevBuf<double> tw0[3][3], tw1[3][3];  // the rows behind ft, [kind][axis]
  fl::DevBuf<int>    tc0[3][3];
  fl::DevBuf<double> bws[3];
  fl::DevBuf<double> stabs[2][3];  // scaled tables: [0] the handle's coefficients, [1] fl_momentum_rhs
  fl::DevBuf<double> srhs;         // Schur right-hand side of fl_abf_apply
  fl::DevBuf<double> gr, gd;       // -ksp_initial_guess_nonzero: b - A x0 and the correction (3*cells each, unpadded)
  fl::DevBuf<double> tmpv;         // 3*cells scratch of fl_abf_jacobian_mult
  fl::DevBuf<double> F;            // 12 padded face fields: V0[0..2], v0interp[c*3+d] at 3 + c*3 + d
  fl::DevBuf<double> dg;           // diag(A), 3 padded components (valid after set_state)
  fl::DevBuf<double> v0p;          // v0 (3 padded components with valid ghosts) when the state came through fl_momentum_set_state_v0
  bool               fly = false;  // k_mom3: v0interp on inner faces is interpolated from v0p inside the kernel
  fl::DevBuf<double> vec[8];
  // PCABF with schurainv / upperainv != ID (abfpc.c:81-94, 151-171): 1 / diag(A) or 1 / rowsum(A), scratch, FGMRES basis
  int                             schur_ainv = FL_ABF_AINV_ID, upper_ainv = FL_ABF_AINV_ID;
  fl::DevBuf<double>              ainv[2], zV[3], gv;
  std::vector<fl::DevBuf<double>> gm;  // cell vectors of the Schur solve with a variable-coefficient S
  std::vector<fl::DevBuf<double>> kb;  // KSPGMRES on A: Krylov basis (3*cells each, allocated as the iteration needs them), w, x, r
  bool   have_state = false;
  double dmean = 1.;   // mean_i a_ii, formed with gersh
  double gersh = -1.;  // cached Gershgorin radius of the Jacobi-scaled operator (fl_momentum_gershgorin); < 0: not computed for this state
  int    t2x = 1, t2chunk = 1, t2zc = 1, t2blocks = 1;  // 128 x 8 x t2zc tiles of k_mom2 / k_mom3 / k_mom_pw3 (mom_plan); t2blocks = entries of their partial sums
};

namespace fl {

// blocks of 256 threads for a grid-stride loop over n entries
inline int nblk_flat(int64_t n) { return (int)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, 8192)); }

// k_mom3 (v0interp of the inner faces formed in the kernel) runs when the state came with v0 (fl_momentum_set_state_v0) and ny > 8: no 128 x 8
// tile then holds both ends of the y axis (k_mom3 stages one block-end row); else k_mom2, all twelve face fields read
inline bool mom3_grid(const GridP &g) { return g.ny > 8; }

// ---- fl_momentum.hip.  The launchers go on the handle's stream and leave hipGetLastError to the caller, where it always was; one asked for a
// combination of template arguments that the library does not hold returns FL_ERR_SUP and launches nothing.
int mom_vec(fl_momentum *m, int slot);         // work vector `slot` (three padded components), made on first use
int mom_ghosts(fl_momentum *m, double *v3);    // ghost layers of three padded components
int mom_stage(fl_momentum *m, const double *v_dev);  // the caller's three unpadded components into vec[7], ghosts filled: what a product reads
// y = A x by k_mom2 / k_mom3<8, dot, jac, out, 1>.  dot: 0 no inner products, 1 sum y and y.o (slots 0, 1), 2 x.y and y.y (slots 2, 3); jac: y = D^-1 A x;
// out: 0 padded y, 1 unpadded y, 2 the diagonal, 3 the off-diagonal row sums
int mom_launch_apply(fl_momentum *m, int dot, bool jac, int out, const double *x, double *y, const double *o, const KspScal *s);
// one fused Chebyshev step, k_mom3<8, 0, jac, 4, 1> (only where m->fly && mom3_grid): xout holds x_{k-1} and receives x_{k+1}
void mom_launch_cheb_step(fl_momentum *m, bool jac, const double *xin, double *xout, const double *b);
int  mom_launch_pw(fl_momentum *m, int op, const double *a0, const double *a1, const double *a2, const double *a3, double *w0, double *w1);  // k_mom_pw3<op>, op 0 .. 6

// ---- fl_vec.hip: y = a x + b z on the handle's stream (z may be NULL; y may alias x or z)
void lincomb(fl_poisson *h, int64_t n, double a, const double *x, double b, const double *z, double *y);

}  // namespace fl

#pragma GCC visibility pop
