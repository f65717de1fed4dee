"""Time the Boussinesq term of the momentum right-hand side (fl_momentum_add_buoyancy, k_buoyancy of fl_buoyancy.hip) at N^3 with HIP events -- inputs
resident, warm-up, the spread over the repeats -- for one scalar under gravity along one axis (8 + 16 = 24 B/cell compulsory) and for three scalars
under gravity along three axes (24 + 48 = 72 B/cell), beside, in the same process, the box's own copy rate (a device-to-device copy of one field:
16 B/cell) and the fl_vec_lincomb calls that compose the same update without the kernel: one call  momrhs_d += (dt a_s,d) phi_s  per scalar and
active component (24 B/cell each) and one call per active component for the constant  -dt sum_s a_s,d ref_s  times a field of ones (24 B/cell) --
fl_vec_lincomb has no constant term.  The composition is timed with and without the constant's calls (ref = 0 needs none).  The copy is timed
twice, before and after: the spread of its two medians is the noise floor.  No pass / fail number: profiles/buoyancy.txt.

usage: python tools/buoyancy_bench.py [--cells 512] [--reps 20] [--out FILE]"""
import argparse
import ctypes as C
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch

from fluca_amd import capi
from fluca_amd.poisson import Momentum, Poisson
from oracle import fluca_oracle as fo
from tools.scalar_bench import line, timed

DT = 2e-3
CASES = [("one scalar, gravity along y", [[0.0, 9.81 * 2.0, 0.0]], [0.5]),
         ("three scalars, gravity along x, y and z", [[1.5, 19.62, -0.7], [-0.4, 4.9, 0.3], [2.2, -9.81, 1.1]], [0.5, 0.1, -0.2])]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, nargs="+", default=[512])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "buoyancy_bench.py needs a GPU"
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    lines = [f"tools/buoyancy_bench.py --cells {' '.join(map(str, a.cells))} --reps {a.reps}   ({torch.cuda.get_device_name(0)})"]
    ptr = lambda t: C.c_void_p(t.data_ptr())
    for n in a.cells:
        xf = [np.linspace(0.0, 1.0, n + 1) for _ in range(3)]
        P = Poisson((n, n, n), xf, [fo.BC_VELOCITY] * 6, DT)
        P.set_stream(stream)
        M = Momentum(P)
        N = n ** 3
        g = torch.Generator(device="cuda").manual_seed(3)
        rnd = lambda m: torch.rand(m, dtype=torch.float64, device="cuda", generator=g) - 0.5
        momrhs, phis, ones, spare = rnd(3 * N), [rnd(N) + 0.5 for _ in range(3)], torch.ones(N, dtype=torch.float64, device="cuda"), torch.empty(N, dtype=torch.float64, device="cuda")
        lines.append(f"{n}^3 cells ({N * 8 / 2 ** 30:.2f} GiB a field), dt {DT}, random momrhs and phi, HIP events around each call or group of calls")
        copy1 = timed(lambda: spare.copy_(phis[0]), a.reps)
        lines.append(line("device-to-device copy of one field, first run", copy1, 16, N))
        results = []
        for what, accel, refs in CASES:
            ns = len(accel)
            act = [d for d in range(3) if any(accel[s][d] != 0.0 for s in range(ns))]
            nbytes = 8 * ns + 16 * len(act)

            def composed(with_constant):
                for d in act:
                    md = momrhs[d * N:(d + 1) * N]
                    for s in range(ns):
                        if accel[s][d] != 0.0:
                            capi.check(capi.lib.fl_vec_lincomb(P.h, N, 1.0, ptr(md), DT * accel[s][d], ptr(phis[s]), ptr(md)), "fl_vec_lincomb")
                    if with_constant:
                        capi.check(capi.lib.fl_vec_lincomb(P.h, N, 1.0, ptr(md), -DT * sum(accel[s][d] * refs[s] for s in range(ns)), ptr(ones), ptr(md)), "fl_vec_lincomb")
            ncalls = sum(1 for d in act for s in range(ns) if accel[s][d] != 0.0)
            one = timed(lambda: M.add_buoyancy(momrhs, phis[:ns], accel, refs, DT), a.reps)
            comp0 = timed(lambda: composed(False), a.reps)
            comp1 = timed(lambda: composed(True), a.reps)
            lines.append(f" {what}:")
            lines.append(line("fl_momentum_add_buoyancy (one launch)", one, nbytes, N))
            lines.append(line(f"{ncalls} x fl_vec_lincomb (ref = 0)", comp0, 24 * ncalls, N))
            lines.append(line(f"{ncalls + len(act)} x fl_vec_lincomb (with the constant)", comp1, 24 * (ncalls + len(act)), N))
            results.append((what, statistics.median(one), statistics.median(comp0), statistics.median(comp1), nbytes))
        copy2 = timed(lambda: spare.copy_(phis[0]), a.reps)
        lines.append(line("device-to-device copy of one field, second run", copy2, 16, N))
        c1, c2 = statistics.median(copy1), statistics.median(copy2)
        base = 0.5 * (c1 + c2)
        lines.append(f"  noise floor: the two copy runs' medians differ by {abs(c1 - c2):.4f} ms = {abs(c1 - c2) / base:.2%} of their mean {base:.4f} ms")
        for what, one, comp0, comp1, nbytes in results:
            lines.append(f"  {what}: one launch / composition = {one / comp0:.3f} (ref = 0), {one / comp1:.3f} (with the constant); "
                         f"{nbytes * N / one / (16 * N / base):.1%} of the copy rate")
        M.close()
        P.close()
        del momrhs, phis, ones, spare
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
