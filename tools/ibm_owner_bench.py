"""Time one fl_ibm_interp + fl_ibm_spread pair with replicated and with owner-rank markers on a 2 x 2 x 2 in-process rank grid (eight handles, eight
host threads, ONE device, the in-memory wire of tests/plugins/inproc_comm.c).  Each rank holds an NX x NY x NZ block (default 256 x 256 x 128); the
markers are config 5's cylinder (diameter 64 h along the periodic span, one ring of 201 markers per z plane) where the four x-y blocks meet.
HIP events on every rank's stream around a warmed window of `reps` pairs, the two modes alternated `rounds` times in one call.

What the number is: the kernel-work side only -- own + ghost wavefronts against L wavefronts per rank, on a device the eight ranks share.
What it is not: the host-staged wire (a stream wait and two copies through pinned memory per exchange or all-reduce) says nothing about the
latency between GPUs, which is what decides between the two modes there.
usage: python tools/ibm_owner_bench.py [NX NY NZ] [reps] [rounds]"""
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch

from fluca_amd import capi
from fluca_amd.poisson import Poisson
from tests import inproc
from tests import mp_common as mpc

blk = tuple(int(a) for a in sys.argv[1:4]) if len(sys.argv) > 3 else (256, 256, 128)
reps = int(sys.argv[4]) if len(sys.argv) > 4 else 20
rounds = int(sys.argv[5]) if len(sys.argv) > 5 else 3
ranks = (2, 2, 2)
n = tuple(blk[d] * ranks[d] for d in range(3))
h = 1.0 / n[0]
box = [(0.0, n[d] * h) for d in range(3)]
bc = [1, 2, 1, 1, 3, 3]      # VELOCITY inlet, PRESSURE_OUTLET, walls, periodic span


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
    with torch.cuda.stream(s):
        L = X[0].size
        Xd = [torch.as_tensor(a, device="cuda") for a in X]
        idx, cnt = torch.zeros(L, dtype=torch.int64, device="cuda"), C.c_int64()
        capi.check(lib.fl_ibm_owned_select(P.h, 0, L, *[ptr(t) for t in Xd], ptr(idx), C.byref(cnt)))
        sel = idx[:cnt.value].clone()
        Xl = [t[sel].contiguous() for t in Xd]
        Lo = int(sel.numel())
        sets = {"replicated": C.c_void_p(), "owner": C.c_void_p()}
        capi.check(lib.fl_ibm_create(P.h, 0, L, *[ptr(t) for t in Xd], C.byref(sets["replicated"])))
        capi.check(lib.fl_ibm_create_owned(P.h, 0, Lo, *[ptr(t) for t in Xl], ptr(sel), C.byref(sets["owner"])))
        c5 = (C.c_int64 * 5)()
        capi.check(lib.fl_ibm_owned_counts(sets["owner"], c5))
        u = torch.rand(3 * P.ncell, dtype=torch.float64, device="cuda")
        f = torch.zeros(3 * P.ncell, dtype=torch.float64, device="cuda")
        arg = {}
        for name, m in (("replicated", L), ("owner", Lo)):
            arg[name] = (torch.empty(3 * m, dtype=torch.float64, device="cuda"), torch.rand(3 * m, dtype=torch.float64, device="cuda"),
                         torch.full((m,), h ** 3, dtype=torch.float64, device="cuda"))

        def pair(name):
            U, F, dV = arg[name]
            capi.check(lib.fl_ibm_interp(sets[name], 3, ptr(u), ptr(U)))
            capi.check(lib.fl_ibm_spread(sets[name], 3, ptr(F), ptr(dV), ptr(f)))

        ms = {"replicated": [], "owner": []}
        for _ in range(rounds):
            for name in ("replicated", "owner"):
                pair(name)      # warm: buffers of the mode, pinned staging of the wire
                s.synchronize()
                R.barrier()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(s)
                for _ in range(reps):
                    pair(name)
                e1.record(s)
                s.synchronize()
                ms[name].append(e0.elapsed_time(e1) / reps)
                R.barrier()
        for m in sets.values():
            lib.fl_ibm_destroy(m)
    P.close()
    return dict(rank=R.rank, owned=c5[0], ghosts=c5[1], copies=c5[2], ms_per_pair={k: [round(v, 4) for v in vs] for k, vs in ms.items()})


X = markers()
res = inproc.run_threads(8, worker, X, timeout=900.0, wire_timeout=120.0)
print(json.dumps(dict(block=blk, ranks=ranks, markers=int(X[0].size), reps=reps, rounds=rounds, wire="host-staged, in-process", delta="peskin4")))
for r in res:
    print(json.dumps(r))
best = {k: max(min(r["ms_per_pair"][k]) for r in res) for k in ("replicated", "owner")}
print(json.dumps(dict(slowest_rank_best_round_ms_per_pair=best, wavefronts_per_rank=dict(replicated=int(X[0].size), owner=max(r["owned"] + r["ghosts"] for r in res)))))
