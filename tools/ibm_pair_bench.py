#!/usr/bin/env python3
"""Config 4's IBM pair alone -- fl_ibm_interp + fl_ibm_spread of three components on the 512^3 grid, sphere D = 64 h, 12 868 markers, Peskin --
timed with HIP events: 7 batches of 200 stream-ordered pairs, microseconds per pair and their median as one JSON line.

    python tools/ibm_pair_bench.py                                  # the library of this tree
    FLUCA_LIB_DIR=<dir with another libflucahip.so> python tools/ibm_pair_bench.py      # e.g. the parent commit's, alternately in one visit
"""
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch

import fluca_amd.poisson as flp
from fluca_amd import capi
n = 512
P = flp.Poisson.uniform((n,) * 3, [(0, 1), (0, 1), (0, 1)], [1] * 6, 1e-3)
stream = torch.cuda.Stream(); P.set_stream(stream)
h = 1.0 / n; R = 32 * h
L = int(round(4 * np.pi * R * R / (h * h)))
i = np.arange(L) + 0.5
phi, th = np.arccos(1 - 2 * i / L), np.pi * (1 + 5 ** 0.5) * i
X = [torch.as_tensor(a, device="cuda") for a in (0.5 + R * np.cos(th) * np.sin(phi), 0.5 + R * np.sin(th) * np.sin(phi), 0.5 + R * np.cos(phi))]
u = torch.rand(3 * P.ncell, dtype=torch.float64, device="cuda"); F = torch.rand(3 * L, dtype=torch.float64, device="cuda")
dV = torch.full((L,), h ** 3, dtype=torch.float64, device="cuda"); U = torch.empty(3 * L, dtype=torch.float64, device="cuda")
f = torch.zeros(3 * P.ncell, dtype=torch.float64, device="cuda")
ptr = lambda t: C.c_void_p(t.data_ptr())
m = C.c_void_p(); torch.cuda.synchronize()
capi.check(capi.lib.fl_ibm_create(P.h, capi.DELTA_PESKIN4, L, ptr(X[0]), ptr(X[1]), ptr(X[2]), C.byref(m)), "fl_ibm_create")
def step():
    capi.check(capi.lib.fl_ibm_interp(m, 3, ptr(u), ptr(U))); capi.check(capi.lib.fl_ibm_spread(m, 3, ptr(F), ptr(dV), ptr(f)))
for _ in range(20): step()
P.synchronize()
out = []
with torch.cuda.stream(stream):
    for b in range(7):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(200): step()
        e1.record(stream); e1.synchronize()
        out.append(e0.elapsed_time(e1) / 200 * 1e3)
capi.lib.fl_ibm_destroy(m); P.close()
print(json.dumps({"lib": os.environ.get("FLUCA_LIB_DIR", "tree"), "markers": L, "us_per_pair": [round(x, 2) for x in out], "median": round(float(np.median(out)), 2)}))
