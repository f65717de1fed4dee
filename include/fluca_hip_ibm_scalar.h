/* fluca_hip_ibm_scalar.h -- a scalar held at a value on the markers of an immersed body (a heated sphere or cylinder), and the scalar content the
 * body hands to the fluid.  An addition to fluca_hip.h (included below), which declares fl_ibm and the error classes; FL_ABI_VERSION does not
 * change, no struct of fluca_hip.h does.
 *
 * The operation is multi-direct forcing of one cell field phi.  phi^(0) is the caller's phi, T_l the target at marker l; for k = 1 .. npass
 *
 *   Phi_l   = interp(phi^(k-1))_l              the value fl_ibm_interp(m, 1, .) gives
 *   q_l     = T_l - Phi_l                      rounded once
 *   Q_l     = q_l (k = 1),  Q_l + q_l (k > 1)  rounded once
 *   phi^(k) = phi^(k-1) + spread(q, dV)        what fl_ibm_spread(m, 1, q, dV, phi) adds, in its order (ascending marker number per cell)
 *
 * THE CONTRACT IS BITWISE: on every marker distribution (replicated, owner rank with ghost markers, after fl_ibm_migrate) and every rank grid the
 * result is exactly fl_ibm_interp(1) -> fl_vec_lincomb(-1 Phi + 1 T) -> fl_ibm_spread(1) per pass through the entry points of fluca_hip.h; Q is
 * the one addition.  On one rank a pass is two launches (the defect is formed in the interpolation's launch, the spread stages one value per
 * marker); on several ranks the messages are those of fl_ibm_interp(1) and fl_ibm_spread(1).
 *
 * Only the surface markers are forced: the body's interior is not held at T.  With dV far above the cell volume the passes need not contract
 * (as for the velocity forcing).  Prescribed-flux (Neumann) bodies are not part of this. */
#ifndef FLUCA_HIP_IBM_SCALAR_H
#define FLUCA_HIP_IBM_SCALAR_H

#include "fluca_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* npass passes of the operation above, phi in place.  Exactly one of target_dev (device, one value per marker of the set: L, or Lo on an
 * owned set) and value (HOST, nbody doubles, read before the call returns) is non-NULL; with value, body_dev (device int32, ids 0..nbody-1,
 * NULL: one body) selects the entry.  The ids MUST be valid: nothing on the device clamps or checks them (fl_ibm_scalar_rate and fl_ibm_force
 * do).  dV_dev as fl_ibm_spread's.  Q_dev (device, L or Lo doubles) may be NULL.  1 <= npass <= 16, 1 <= nbody <= 64.
 * FL_ERR_ARG_NULL: m, phi_dev or (with markers) dV_dev missing; FL_ERR_ARG_OUTOFRANGE: npass or nbody; FL_ERR_ARG_WRONG: both or neither of
 * target_dev and value (a rank of an owned set that holds no marker may pass neither).  On an owned set over several ranks these are voted: every
 * rank returns the error.  Stream-ordered: on one rank enqueues and returns; collective where fl_ibm_interp / fl_ibm_spread are. */
int fl_ibm_scalar_force(fl_ibm *m, int npass, const double *target_dev, const int32_t *body_dev, int nbody, const double *value,
                        const double *dV_dev, double *phi_dev, double *Q_dev);
/* rate[b] = sum over the markers of body b of Q_l dV_l, HOST array of nbody doubles: fl_ibm_force's exact split sum (same bound, same limit of
 * 2^22 markers, NaN rule, voting, collectives) -- bit for bit the first force component fl_ibm_force returns for F = (Q, 0, 0); a body id outside
 * 0..nbody-1 is FL_ERR_ARG_OUTOFRANGE as there.  Waits for the stream.  The bits do not depend on the order of the markers or on how an owned set
 * is shared out; they do depend on Q, which differs at rounding level between rank grids. */
int fl_ibm_scalar_rate(fl_ibm *m, const double *Q_dev, const double *dV_dev, const int32_t *body_dev, int nbody, double *rate);

#ifdef __cplusplus
}
#endif
#endif
