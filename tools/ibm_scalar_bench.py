#!/usr/bin/env python3
"""One fl_ibm_scalar_force call beside the composition it equals bit for bit -- fl_ibm_interp(1), fl_vec_lincomb, fl_ibm_spread(1) per pass -- in one process.

usage: python tools/ibm_scalar_bench.py [--cells 512] [--rounds 9] [--reps 200] [--out profiles/ibm_scalar.txt]
Marker set: config 4's sphere (Fibonacci lattice of diameter 64 h: 12 868 markers at 512^3, tools/ibm_force_bench.py's) on a cells^3 channel block, one
body held at 1 through the value table, npass = 1 and 4.  Both sides are stream-ordered, so a timed window is `reps` calls back to back between two HIP
events on the handle's stream (the stream never idles: what a time step pays); the rounds of the two sides alternate.  The figure to hold the fused call
against is the composition's own spread over its rounds: median, minimum, maximum, and (max - min) / median are written next to the numbers.  Before the
timing the two sides are compared bit for bit at the size timed.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.ibm_force_bench import sphere  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out", type=str, default="")
    a = ap.parse_args()
    from fluca_amd import capi
    from fluca_amd import poisson as flp
    lib = capi.lib
    n = a.cells
    h = 1.0 / n
    P = flp.Poisson.uniform((n, n, n), [(0, 1)] * 3, [1, 2, 1, 1, 3, 3], 1e-3)
    stream = torch.cuda.Stream()
    P.set_stream(stream)
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    rows = []
    with torch.cuda.stream(stream):
        Xh = sphere(n, h)
        L = Xh[0].size
        X = [torch.as_tensor(v, device="cuda") for v in Xh]
        dV = torch.full((L,), h ** 3, dtype=torch.float64, device="cuda")
        T = torch.ones(L, dtype=torch.float64, device="cuda")
        phi0 = torch.rand(P.ncell, dtype=torch.float64, device="cuda")
        phi, Phi, q, Q = phi0.clone(), torch.empty_like(T), torch.empty_like(T), torch.empty_like(T)
        hm = C.c_void_p()
        stream.synchronize()
        capi.check(lib.fl_ibm_create(P.h, capi.DELTA_PESKIN4, L, ptr(X[0]), ptr(X[1]), ptr(X[2]), C.byref(hm)), "fl_ibm_create")
        one = (C.c_double * 1)(1.0)

        def fused(npass):
            capi.check(lib.fl_ibm_scalar_force(hm, npass, None, None, 1, one, ptr(dV), ptr(phi), ptr(Q)))

        def composition(npass):
            for _ in range(npass):
                capi.check(lib.fl_ibm_interp(hm, 1, ptr(phi), ptr(Phi)))
                capi.check(lib.fl_vec_lincomb(P.h, L, -1.0, ptr(Phi), 1.0, ptr(T), ptr(q)))
                capi.check(lib.fl_ibm_spread(hm, 1, ptr(q), ptr(dV), ptr(phi)))

        def window(fn, npass):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            stream.synchronize()
            e0.record(stream)
            for _ in range(a.reps):
                fn(npass)
            e1.record(stream)
            e1.synchronize()
            return e0.elapsed_time(e1) / a.reps * 1e3        # microseconds per call

        for npass in (1, 4):
            # the same bits, at the size timed
            phi.copy_(phi0)
            fused(npass)
            stream.synchronize()
            got = phi.clone()
            phi.copy_(phi0)
            composition(npass)
            stream.synchronize()
            same = bool(torch.equal(got.view(torch.int64), phi.view(torch.int64)))
            for fn in (fused, composition):                   # warm-up
                for _ in range(10):
                    fn(npass)
            t = {"fused": [], "composition": []}
            for _ in range(a.rounds):
                phi.copy_(phi0)
                t["composition"].append(window(composition, npass))
                phi.copy_(phi0)
                t["fused"].append(window(fused, npass))
            row = dict(set="config 4 sphere", markers=L, cells=n, npass=npass, rounds=a.rounds, reps=a.reps, same_bits=same)
            for k, v in t.items():
                med = statistics.median(v)
                row[k + "_us"] = dict(median=round(med, 2), min=round(min(v), 2), max=round(max(v), 2), spread=round((max(v) - min(v)) / med, 3))
            row["fused_over_composition"] = round(row["fused_us"]["median"] / row["composition_us"]["median"], 3)
            row["fused_not_slower_beyond_the_spread"] = bool(row["fused_us"]["median"] <= row["composition_us"]["median"] * (1 + row["composition_us"]["spread"]))
            rows.append(row)
            print(json.dumps(row), flush=True)
        lib.fl_ibm_destroy(hm)
    P.close()
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("# python tools/ibm_scalar_bench.py " + " ".join(sys.argv[1:]) + "\n")
            fh.write("# microseconds per call between two HIP events around `reps` calls back to back (median / min / max over the rounds, spread = (max - min) / median); "
                     + capi.lib.fl_version().decode() + "\n")
            for row in rows:
                fh.write(json.dumps(row) + "\n")
    if not all(r["same_bits"] for r in rows):
        sys.exit("fl_ibm_scalar_force and the composition differ")


if __name__ == "__main__":
    main()
