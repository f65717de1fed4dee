#!/usr/bin/env python3
"""One fl_ibm_force call (force + torque, one body) beside the fl_ibm_interp + fl_ibm_spread pair of the same marker set, in one process.

usage: python tools/ibm_force_bench.py [--cells 512] [--rounds 7] [--reps 20] [--out profiles/ibm_force.txt]
Marker sets: config 4's sphere (Fibonacci lattice of diameter 64 h: 12 868 markers) and config 5's marker count (102 944, on cylinders along z),
on a cells^3 channel block.  fl_ibm_force waits for the device before it returns (its result is on the host), so it is timed per call by the wall
clock; interp and spread are stream-ordered, so they are timed both ways: back to back (the stream never idles: what a time step pays for them)
and one call followed by a wait (what the force call is comparable with).  Rounds of the three are interleaved; median and minimum over the rounds.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def sphere(n, h):
    R = 32 * h
    L = int(round(4 * np.pi * R * R / (h * h)))
    i = np.arange(L) + 0.5
    phi, th = np.arccos(1 - 2 * i / L), np.pi * (1 + 5 ** 0.5) * i
    return [0.5 + R * np.cos(th) * np.sin(phi), 0.5 + R * np.sin(th) * np.sin(phi), 0.5 + R * np.cos(phi)]


def cylinders(n, h, L):
    nth = int(round(2 * np.pi * 32))
    m = np.arange(L)
    th = (m % nth + 0.5) * 2 * np.pi / nth
    ring = m // nth
    rad = (32 + 3 * (ring // n)) * h
    return [0.5 + rad * np.cos(th), 0.5 + rad * np.sin(th), ((ring % n) + 0.5) * h]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", type=str, default="")
    a = ap.parse_args()
    from fluca_amd import capi
    from fluca_amd import poisson as flp
    lib = capi.lib
    n = a.cells
    h = 1.0 / n
    P = flp.Poisson.uniform((n, n, n), [(0, 1)] * 3, [1, 2, 1, 1, 3, 3], 1e-3)
    u = torch.rand(3 * P.ncell, dtype=torch.float64, device="cuda")
    f = torch.zeros(3 * P.ncell, dtype=torch.float64, device="cuda")
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    rows = []
    for name, Xh in (("config 4 sphere", sphere(n, h)), ("config 5 marker count", cylinders(n, h, 102944))):
        L = Xh[0].size
        X = [torch.as_tensor(v, device="cuda") for v in Xh]
        F = torch.rand(3 * L, dtype=torch.float64, device="cuda") - 0.5
        dV = torch.full((L,), h ** 3, dtype=torch.float64, device="cuda")
        U = torch.empty(3 * L, dtype=torch.float64, device="cuda")
        hm = C.c_void_p()
        torch.cuda.synchronize()
        capi.check(lib.fl_ibm_create(P.h, capi.DELTA_PESKIN4, L, ptr(X[0]), ptr(X[1]), ptr(X[2]), C.byref(hm)), "fl_ibm_create")
        about, force, torque = (C.c_double * 3)(0.5, 0.5, 0.5), (C.c_double * 3)(), (C.c_double * 3)()
        calls = {
            "force": lambda: capi.check(lib.fl_ibm_force(hm, ptr(F), ptr(dV), None, 1, about, force, torque)),
            "interp": lambda: capi.check(lib.fl_ibm_interp(hm, 3, ptr(u), ptr(U))),
            "spread": lambda: capi.check(lib.fl_ibm_spread(hm, 3, ptr(F), ptr(dV), ptr(f))),
        }

        def back_to_back(fn):
            P.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.reps):
                fn()
            P.synchronize()
            return (time.perf_counter() - t0) / a.reps * 1e6

        def with_wait(fn):
            P.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.reps):
                fn()
                P.synchronize()
            return (time.perf_counter() - t0) / a.reps * 1e6

        for fn in calls.values():      # warm-up: first launches, the force workspace
            fn()
        P.synchronize()
        t = {k: [] for k in ("force", "interp", "spread", "interp+wait", "spread+wait")}
        for _ in range(a.rounds):
            t["force"].append(back_to_back(calls["force"]))
            t["interp"].append(back_to_back(calls["interp"]))
            t["spread"].append(back_to_back(calls["spread"]))
            t["interp+wait"].append(with_wait(calls["interp"]))
            t["spread+wait"].append(with_wait(calls["spread"]))
        row = dict(set=name, markers=L, cells=n, rounds=a.rounds, reps=a.reps, force=list(force), torque=list(torque))
        for k, v in t.items():
            row[k + "_us"] = dict(median=round(statistics.median(v), 2), min=round(min(v), 2), max=round(max(v), 2))
        row["force_over_interp"] = round(row["force_us"]["median"] / row["interp_us"]["median"], 3)
        row["force_over_interp_with_wait"] = round(row["force_us"]["median"] / row["interp+wait_us"]["median"], 3)
        row["force_over_pair_with_wait"] = round(row["force_us"]["median"] / (row["interp+wait_us"]["median"] + row["spread+wait_us"]["median"]), 3)
        rows.append(row)
        lib.fl_ibm_destroy(hm)
        print(json.dumps(row), flush=True)
    P.close()
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("# python tools/ibm_force_bench.py " + " ".join(sys.argv[1:]) + "\n")
            fh.write("# microseconds per call (median / min / max over the rounds); " + capi.lib.fl_version().decode() + "\n")
            for row in rows:
                fh.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
