"""Time fl_abf_schur_apply with schurainv = DIAG on a 2 x 1 x 1 in-process rank grid (two handles, two host threads, one device, the in-memory wire
of tests/plugins/inproc_comm.c): each rank holds an NX x NY x NZ block (default 512 x 512 x 256, config 5's block).  The one-pass product on
several ranks (k_schur_var_ring + the two-deep exchange of p + the ring of a^-1) against the composition of seven kernels, and the one-rank
product of one block alone for the cost of the exchanges.  The two ranks share the device, so their products run at the same time.
usage: python tools/schur_var_mr_bench.py [NX NY NZ] [reps]"""
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch

from fluca_amd import capi
from fluca_amd.poisson import Momentum, Poisson
from oracle import fluca_oracle as fo
from tests import inproc
from tests import mp_common as mpc

blk = tuple(int(a) for a in sys.argv[1:4]) if len(sys.argv) > 3 else (512, 512, 256)
reps = int(sys.argv[4]) if len(sys.argv) > 4 else 10
V, O, PER = fo.BC_VELOCITY, fo.BC_PRESSURE_OUTLET, fo.BC_PERIODIC
bc = [V, O, V, V, PER, PER]


def session(R, ranks):
    n = (blk[0] * ranks[0], blk[1], blk[2])
    xf = [np.linspace(0.0, 1.0, n[d] + 1) for d in range(3)]
    d = mpc.decomp_of(capi, n, ranks, R.rank) if R is not None else None
    P = Poisson(n, xf, bc, 1e-3, decomp=d)
    s = torch.cuda.Stream()
    P.set_stream(s)
    if R is not None:
        R.attach(P.h)
    return P, s


def worker(R, ranks, mode):
    P, s = session(R, ranks)
    with torch.cuda.stream(s):
        M = Momentum(P)
        N = P.ncell
        g = torch.Generator(device="cuda").manual_seed(3 + (0 if R is None else R.rank))
        rnd = lambda m: torch.rand(m, dtype=torch.float64, device="cuda", generator=g) - 0.5
        V0 = [8.0 * rnd(P.nface[d]) for d in range(3)]
        W = [8.0 * rnd(P.nface[d]) for c in range(3) for d in range(3)]
        M.set_state(1e-3, 1.0, 0.05, V0, W)
        M.set_ainv_types(schur=fo.AINV_DIAG)
        p = rnd(N)
        y = M.schur_apply(p)
        s.synchronize()
        if R is not None:
            R.barrier()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            y = M.schur_apply(p)
            s.synchronize()
            ts.append(time.perf_counter() - t0)
        M.close()
    P.close()
    return float(np.median(ts))


out = {}
for mode in (1, 0):
    capi.check(capi.lib.fl_tuning_set(b"schur_var_fused", mode))
    try:
        out[mode] = inproc.run_threads(2, worker, (2, 1, 1), mode)
        out[("one", mode)] = inproc.run_threads(1, lambda R: worker(None, (1, 1, 1), mode))[0]
    finally:
        capi.check(capi.lib.fl_tuning_set(b"schur_var_fused", 1))
f, c = out[1], out[0]
print(f"block {blk[0]}x{blk[1]}x{blk[2]} per rank, 2 x 1 x 1 ranks on one device, median of {reps} products, a^-1 = 1/diag(A) recomputed in each "
      f"(fl_abf_schur_apply)")
print(f"  2 ranks, one pass:     rank 0 {f[0] * 1e3:.3f} ms  rank 1 {f[1] * 1e3:.3f} ms")
print(f"  2 ranks, composition:  rank 0 {c[0] * 1e3:.3f} ms  rank 1 {c[1] * 1e3:.3f} ms   ratio {max(c) / max(f):.2f}")
print(f"  1 rank (the block alone): one pass {out[('one', 1)] * 1e3:.3f} ms  composition {out[('one', 0)] * 1e3:.3f} ms")
