"""Time one fl_ibm_migrate of config 5's cylinder on a 2 x 2 x 2 in-process rank grid (eight handles, eight host threads, ONE device, the in-memory
wire of tests/plugins/inproc_comm.c) against what it replaces: re-partitioning the replicated list and creating a new set (fl_ibm_owned_select +
fl_ibm_create_owned) from the same positions.  Blocks and markers are those of tools/ibm_owner_bench.py; the cylinder steps one cell along x and y
back and forth across both split planes, four attributes travel (what the host mirror's moving body carries).

Per rank and repetition, host wall time between a stream synchronisation and a barrier before and a stream synchronisation after (the calls wait for
their own counts, so events on the stream would leave the host's share out):
  migrate         fl_ibm_migrate
  update          fl_ibm_update on the same set at the positions it now holds: the unchanged routing step (ibm_route) that ends a migrate too
  select+create   fl_ibm_owned_select on the replicated list at the new positions + fl_ibm_create_owned (destroying the old set is not timed)
migrate - update is the share of the new kernels and their two exchanges.  The wire is host-staged: nothing here speaks about latency between GPUs.
usage: python tools/ibm_migrate_bench.py [NX NY NZ] [reps]"""
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch

from fluca_amd import capi
from fluca_amd.poisson import Poisson
from tests import inproc
from tests import mp_common as mpc

blk = tuple(int(a) for a in sys.argv[1:4]) if len(sys.argv) > 3 else (256, 256, 128)
reps = int(sys.argv[4]) if len(sys.argv) > 4 else 6
ranks = (2, 2, 2)
n = tuple(blk[d] * ranks[d] for d in range(3))
h = 1.0 / n[0]
box = [(0.0, n[d] * h) for d in range(3)]
bc = [1, 2, 1, 1, 3, 3]      # VELOCITY inlet, PRESSURE_OUTLET, walls, periodic span
NATTR = 4


def markers():
    R = 32 * h
    nth = int(round(2 * np.pi * R / h))
    th = (np.arange(nth) + 0.5) * 2 * np.pi / nth
    z = (np.arange(n[2]) + 0.5) * h
    cx, cy = 0.5 * box[0][1], 0.5 * box[1][1]
    return [np.tile(cx + R * np.cos(th), n[2]), np.tile(cy + R * np.sin(th), n[2]), np.repeat(z, nth)]


def worker(R, X):
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t.numel() else None  # noqa: E731
    lib = capi.lib
    xf = [np.linspace(box[d][0], box[d][1], n[d] + 1) for d in range(3)]
    P = Poisson(n, xf, bc, 1e-3, decomp=mpc.decomp_of(capi, n, ranks, R.rank))
    s = torch.cuda.Stream()
    P.set_stream(s)
    R.attach(P.h)
    out = dict(rank=R.rank, migrate_ms=[], update_ms=[], select_create_ms=[], moved=[], own=[])

    def timed(fn):
        s.synchronize()
        R.barrier()
        t0 = time.perf_counter()
        fn()
        s.synchronize()
        return 1e3 * (time.perf_counter() - t0)

    with torch.cuda.stream(s):
        L = X[0].size
        base = [torch.as_tensor(a, device="cuda") for a in X]

        def select_create(Xd):
            idx, cnt = torch.zeros(L, dtype=torch.int64, device="cuda"), C.c_int64()
            capi.check(lib.fl_ibm_owned_select(P.h, 0, L, *[ptr(t) for t in Xd], ptr(idx), C.byref(cnt)))
            sel = idx[:cnt.value].clone()
            Xl = [t[sel].contiguous() for t in Xd]
            m = C.c_void_p()
            capi.check(lib.fl_ibm_create_owned(P.h, 0, int(sel.numel()), *[ptr(t) for t in Xl], ptr(sel), C.byref(m)))
            return m, sel

        m, gid = select_create(base)
        attr = torch.rand(NATTR * int(gid.numel()), dtype=torch.float64, device="cuda")
        for k in range(reps + 1):      # the first repetition warms buffers and the wire's staging; it is dropped below
            shift = h if k % 2 == 0 else 0.0
            Xd = [base[0] + shift, base[1] + shift, base[2]]
            Xl = [t[gid].contiguous() for t in Xd]
            Lnew, moved = C.c_int64(), (C.c_int64 * 2)()
            ms = timed(lambda: capi.check(lib.fl_ibm_migrate(m, *[ptr(t) for t in Xl], NATTR, ptr(attr), C.byref(Lnew), moved)))
            nl = Lnew.value
            Xf = [torch.empty(nl, dtype=torch.float64, device="cuda") for _ in range(3)]
            gid = torch.empty(nl, dtype=torch.int64, device="cuda")
            attr = torch.empty(NATTR * nl, dtype=torch.float64, device="cuda")
            capi.check(lib.fl_ibm_owned_fetch(m, nl, *[ptr(t) for t in Xf], ptr(gid), NATTR, ptr(attr)))
            ms_u = timed(lambda: capi.check(lib.fl_ibm_update(m, *[ptr(t) for t in Xf])))
            fresh = []
            ms_c = timed(lambda: fresh.append(select_create(Xd)))
            assert torch.equal(fresh[0][1], gid), "the migrated partition is not the fresh one"
            lib.fl_ibm_destroy(fresh[0][0])
            if k:
                out["migrate_ms"].append(round(ms, 3))
                out["update_ms"].append(round(ms_u, 3))
                out["select_create_ms"].append(round(ms_c, 3))
                out["moved"].append(list(moved))
                out["own"].append(nl)
        lib.fl_ibm_destroy(m)
    P.close()
    return out


X = markers()
res = inproc.run_threads(8, worker, X, timeout=900.0, wire_timeout=120.0)
print(json.dumps(dict(block=blk, ranks=ranks, markers=int(X[0].size), reps=reps, attributes=NATTR, wire="host-staged, in-process", delta="peskin4")))
for r in res:
    print(json.dumps(r))
# a collective call ends when its slowest rank does: per repetition the maximum over the ranks, then the median over the repetitions
med = {k: float(np.median(np.max([r[k] for r in res], axis=0))) for k in ("migrate_ms", "update_ms", "select_create_ms")}
print(json.dumps(dict(slowest_rank_median_ms=med, new_kernels_and_exchanges_ms=round(med["migrate_ms"] - med["update_ms"], 3),
                      moved_per_call_all_ranks=[int(sum(r["moved"][k][0] for r in res)) for k in range(reps)])))
