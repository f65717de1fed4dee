// fl_knobs.h -- the tuning knobs of libflucahip.so, in one table.
//
// fl_tuning_set / fl_tuning_get (include/fluca_hip.h): process-wide integers, atomics -- handles of several host threads read them while they
// run; set them before the solves they should affect.  Their initial value is the table's default or, if set, the environment variable
// FLUCA_<NAME IN CAPITALS>; the environment is read ONCE, in one place (knob_table_init, fl_knobs.cpp).  Nothing else in the library reads the
// environment, and there is no second build: every other choice is a constant next to the code it steers.
#pragma once
#include <atomic>

// name, default
#define FL_PUBLIC_KNOBS(X)                                                                                                                   \
  X(cheb_fuse, 1)         /* two Chebyshev steps per sweep: 0 never, 1 where it pays (>= 32768 cells per rank), 2 wherever legal */          \
  X(placement, 0)         /* 1: the first solve of a large handle runs the placement search of fl_poisson_tune_placement */                  \
  X(cg_xbatch, 1)         /* CG: the x-updates of a group of cg_xdepth iterations on the group's last one */                                  \
  X(cg_xdepth, 8)         /* CG, one rank, q-free pair: direction buffers in the ring = iterations per x-update (2, 3, 4, 8 or 16) */        \
  X(cheb_zero3, 1)        /* a smoother call from a zero guess on one rank: its first three steps in one sweep (fl_cheb2.hip, Z) */          \
  X(mg_prolong, 1)        /* FL_PC_MG: 1 tri-linear prolongation, 0 piecewise constant */                                                     \
  X(mg_flexible, 1)       /* FL_PC_MG: 1 Polak-Ribiere beta (flexible CG), 0 KSPCG's */                                                      \
  X(mg_coarse, 1)         /* FL_PC_MG: 1 a coarsest level of <= 4096 cells on one rank is solved by one workgroup */                          \
  X(mg_post_smooth, 0)    /* FL_PC_MG: smoothing steps AFTER the coarse correction; 0 = as many as before it (fl_ksp_opts.mg_smooth_its) */           \
  X(schur_var_fused, 1)   /* PCABF schurainv DIAG / ROWSUM on one rank: 1 the product S p in one pass (fl_schur_var.hip), 0 the composition of seven */   \
  X(overlap, 1)           /* several ranks: the exchange of the new residual hidden behind the update kernel; 0 sequential (A/B, tests) */   \
  X(comm_loopback, 0)     /* 1: a single rank sends the ghost layers of its periodic axes to itself through the communicator (tests) */      \
  X(comm_trace, 0)        /* 1: every host-staged exchange / smoother stage on stderr; 2: with a stream wait per stage */                     \
  X(ghost_width, 0)       /* 0 automatic (2 where a neighbouring rank exists, else 1); 1 / 2 forced (tests) */                                \
  X(placement_verbose, 0) /* the placement search narrates on stderr */                                                                       \
  X(placement_vmm, 1)     /* placement arenas in chunk-mapped virtual memory (everything but the chosen window is released) */               \
  X(allreduce, 0)         /* several ranks: 0 RCCL / the host callbacks, 1 the one-shot all-reduce through peer-mapped buffers (fl_oneshot.h) */

namespace fl {

enum Knob : int {
#define X(n, d) K_##n,
  FL_PUBLIC_KNOBS(X)
#undef X
      K_COUNT
};

int         knob(Knob k);              // relaxed atomic load; the first call of the process fills the table from the environment
void        knob_set(Knob k, int v);
int         knob_find(const char *name);  // index in the table, -1 if there is no such knob
const char *knob_name(int k);

}  // namespace fl
