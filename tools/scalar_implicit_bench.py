"""Time the implicit scalar diffusion (fl_scalar_implicit.hip) at N^3 with HIP events, in the manner of tools/scalar_bench.py -- inputs resident, a
warm-up, and ALTERNATING repeats: the candidates of a group take turns, one launch each per round, so that drift of the box lands on all of them
alike; the noise floor printed beside every number is the distance between the medians of its odd and its even rounds.

  kernels   one Chebyshev step (k_scalar_cheb, 40 B/cell compulsory) and its first step (32 B/cell) beside the box's device-to-device copy of one
            field (16 B/cell), fl_scalar_diffusion_apply (16 B/cell) and one stage of k_scalar_stage (fl_scalar_rhs, 40 B/cell); each as a fraction of
            the MEASURED copy rate
  steps     one IMEX step (fl_scalar_step_imex, theta = 1, rtol 1e-6, five explicit stages) at diffusive numbers out[1] = 4, 20 and 200 beside the
            explicit fl_scalar_step with the smallest nstages that is stable at the same number (s - 1 >= out[1])

  --ring    k_scalar_cheb_ring beside k_scalar_cheb on the same 512 x 512 x 256 block, in the same process and the same alternating rounds: rank 0 of a
            1 x 1 x 2 grid (two handles, two threads, the in-memory transport of tests/inproc.py) makes one collective call, so that its slabs are filled,
            and then times ONE launch (fldbg_scalar_cheb_ring_one: no exchange) with and without the fused pack while the peer idles; the yardsticks -- a
            one-rank handle on a grid that IS that block (fldbg_scalar_cheb_one) and the box's copy of one field -- take their turns in the same rounds.
            Time across GPUs is not measured: the transport is the host's memory.

No pass / fail number: profiles/scalar_implicit.txt, profiles/scalar_implicit_ranks.txt.

usage: python tools/scalar_implicit_bench.py [--cells 512] [--reps 10] [--numbers 4 20 200] [--ring] [--out FILE]"""
import argparse
import ctypes as C
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch

from fluca_amd import capi
from fluca_amd.poisson import Poisson
from fluca_amd.scalar import DIRICHLET, NEUMANN, PERIODIC, Scalar
from oracle import fluca_oracle as fo


def alternating(fns, reps, warm=2):
    """fns: {name: callable}.  -> {name: times in ms, in the order of the rounds}; every round launches each candidate once, bracketed by HIP events"""
    for _ in range(warm):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(reps):
        for k, f in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            out[k].append(a.elapsed_time(b))
    return out


def med(ms):
    return statistics.median(ms)


def floor(ms):
    """the noise floor of a series of alternating repeats: |median of the odd rounds - median of the even rounds|"""
    return abs(med(ms[0::2]) - med(ms[1::2])) if len(ms) > 1 else float("nan")


def line(what, ms, extra=""):
    return f"  {what:<52s} median {med(ms):9.4f} ms  (min {min(ms):.4f}, max {max(ms):.4f}, {len(ms)} rounds, noise floor {floor(ms):.4f} ms){extra}"


RING_BLOCK = (512, 512, 256)
RING_BC = (DIRICHLET, NEUMANN, NEUMANN, NEUMANN, NEUMANN, NEUMANN)     # (z is split: a kind behind a rank face is accepted and unused)
RING_VALS = (1.0, 0.0, 0.0, 0.0, 0.0, 0.0)


def _ring_rank(R, reps, result):
    """one rank of the 1 x 1 x 2 grid: both make the handle and one collective call; rank 0 then times the launches alone"""
    from tests import mp_common as mpc
    nx, ny, nz = RING_BLOCK
    n = (nx, ny, 2 * nz)
    N = nx * ny * nz
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    P = Poisson(n, [np.linspace(0.0, 1.0, m + 1) for m in n], [fo.BC_VELOCITY] * 6, 1e-3, decomp=mpc.decomp_of(capi, n, (1, 1, 2), R.rank))
    P.set_stream(stream)
    R.attach(P.h)
    S = Scalar(P, RING_BC, RING_VALS, gamma=1e-3)
    g = torch.Generator(device="cuda").manual_seed(3 + R.rank)
    rnd = lambda m: torch.rand(m, dtype=torch.float64, device="cuda", generator=g) - 0.5
    phi, out, b, d = rnd(N) + 0.5, torch.empty(N, dtype=torch.float64, device="cuda"), rnd(N), torch.zeros(N, dtype=torch.float64, device="cuda")
    c = 20.0 / (6.0 * float(nx) ** 2)
    S.diffusion_apply(c, phi, out=out)          # collective: the slabs are packed, sent and received
    stream.synchronize()
    R.barrier()
    if R.rank == 0:
        ptr = lambda t: C.c_void_p(t.data_ptr())
        ring = capi.lib.fldbg_scalar_cheb_ring_one
        ring.argtypes = [C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_int, C.c_int] + [C.c_void_p] * 4
        one = capi.lib.fldbg_scalar_cheb_one
        one.argtypes = [C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_int] + [C.c_void_p] * 4
        # the one-rank twin: a grid that is the block, the same tables row for row (the block is the low half of z)
        P1 = Poisson(RING_BLOCK, [np.linspace(0.0, 1.0, nx + 1), np.linspace(0.0, 1.0, ny + 1), np.linspace(0.0, 0.5, nz + 1)], [fo.BC_VELOCITY] * 6, 1e-3)
        P1.set_stream(stream)
        S1 = Scalar(P1, RING_BC, RING_VALS, gamma=1e-3)
        result.update(alternating({
            "copy": lambda: out.copy_(phi),
            "one": lambda: capi.check(one(S1.h, c, 0.4, 0.3, 0, ptr(phi), ptr(b), ptr(d), ptr(out)), "fldbg_scalar_cheb_one"),
            "ring": lambda: capi.check(ring(S.h, c, 0.4, 0.3, 0, 0, ptr(phi), ptr(b), ptr(d), ptr(out)), "fldbg_scalar_cheb_ring_one"),
            "pack": lambda: capi.check(ring(S.h, c, 0.4, 0.3, 0, 1, ptr(phi), ptr(b), ptr(d), ptr(out)), "fldbg_scalar_cheb_ring_one"),
            "one1": lambda: capi.check(one(S1.h, c, 0.0, 0.3, 1, ptr(phi), ptr(b), ptr(d), ptr(out)), "fldbg_scalar_cheb_one"),
            "pack1": lambda: capi.check(ring(S.h, c, 0.0, 0.3, 1, 1, ptr(phi), ptr(b), ptr(d), ptr(out)), "fldbg_scalar_cheb_ring_one"),
        }, reps, warm=3))
        S1.close()
        P1.close()
    R.barrier()                                 # (the peer idles until rank 0 is done)
    S.close()
    P.close()


def ring_leg(a, lines):
    from tests import inproc
    nx, ny, nz = RING_BLOCK
    N = nx * ny * nz
    t = {}
    inproc.run_threads(2, _ring_rank, a.reps, t)
    rate = 16 * N / med(t["copy"])
    frac = lambda key, B: f"  {B:3d} B/cell -> {B * N / med(t[key]) / 1e9:6.3f} TB/s = {B * N / med(t[key]) / rate:6.1%} of the copy rate"
    lines.append(f"--ring: one Chebyshev step on a {nx} x {ny} x {nz} block ({N * 8 / 2 ** 30:.2f} GiB a field), S = 20, random fields, HIP events around each launch, "
                 f"{a.reps} alternating rounds after 3 warm-up rounds")
    lines.append(line("device-to-device copy of one field", t["copy"], frac("copy", 16)))
    lines.append(line("k_scalar_cheb<0>, one rank", t["one"], frac("one", 40)))
    lines.append(line("k_scalar_cheb_ring<0>, rank 0 of 1 x 1 x 2", t["ring"], frac("ring", 40)))
    lines.append(line("k_scalar_cheb_ring<0> with the fused pack", t["pack"], frac("pack", 40)))
    lines.append(line("k_scalar_cheb<1> (first step), one rank", t["one1"], frac("one1", 32)))
    lines.append(line("k_scalar_cheb_ring<1> with the fused pack", t["pack1"], frac("pack1", 32)))
    base = med(t["one"])
    lines.append(f"  ring / one rank = {med(t['ring']) / base:.4f}; with the fused pack = {med(t['pack']) / base:.4f}; first step with the pack = {med(t['pack1']) / med(t['one1']):.4f}"
                 "  (the ring block has a rank face at its high z end: one z plane read from the slab, one plane packed)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=512)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--numbers", type=float, nargs="+", default=[4.0, 20.0, 200.0])
    ap.add_argument("--ring", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "scalar_implicit_bench.py needs a GPU"
    if a.ring:
        lines = [f"tools/scalar_implicit_bench.py --ring --reps {a.reps}   ({torch.cuda.get_device_name(0)})"]
        ring_leg(a, lines)
        text = "\n".join(lines)
        print(text)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as fh:
                fh.write(text + "\n")
        return
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    n = a.cells
    N = n ** 3
    lines = [f"tools/scalar_implicit_bench.py --cells {n} --reps {a.reps} --numbers {' '.join(f'{x:g}' for x in a.numbers)}   ({torch.cuda.get_device_name(0)})"]
    V_, PER = fo.BC_VELOCITY, fo.BC_PERIODIC
    xf = [np.linspace(0.0, 1.0, n + 1) for _ in range(3)]
    P = Poisson((n, n, n), xf, [V_, V_, V_, V_, PER, PER], 1e-3)
    P.set_stream(stream)
    g = torch.Generator(device="cuda").manual_seed(3)
    rnd = lambda m: torch.rand(m, dtype=torch.float64, device="cuda", generator=g) - 0.5
    # a channel: Dirichlet x-, Neumann 0 at x+, Neumann in y, periodic z (the case of tools/scalar_bench.py)
    S = Scalar(P, (DIRICHLET, NEUMANN, NEUMANN, NEUMANN, PERIODIC, PERIODIC), (1.0, 0.0, 0.0, 0.0, 0.0, 0.0), limiter="superbee", gamma=1e-3)
    V = [rnd(P.nface[d]) for d in range(3)]
    S.set_velocity(*V)
    phi, out, b, d = rnd(N) + 0.5, torch.empty(N, dtype=torch.float64, device="cuda"), rnd(N), torch.zeros(N, dtype=torch.float64, device="cuda")
    lines.append(f"{n}^3 cells ({N * 8 / 2 ** 30:.2f} GiB a field), channel boundaries, random fields")

    # ---- the kernels
    one = capi.lib.fldbg_scalar_cheb_one
    one.argtypes = [C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_int] + [C.c_void_p] * 4
    ptr = lambda t: C.c_void_p(t.data_ptr())
    h2 = float(n) ** 2
    c = 20.0 / (6.0 * h2)                       # S = c sum_d 2 / h^2 = 20

    def cheb(first):
        return lambda: capi.check(one(S.h, c, 0.4, 0.3, first, ptr(phi), ptr(b), ptr(d), ptr(out)), "fldbg_scalar_cheb_one")
    t = alternating({"copy": lambda: out.copy_(phi), "cheb": cheb(0), "first": cheb(1), "apply": lambda: S.diffusion_apply(c, phi, out=out),
                     "stage": lambda: S.rhs(phi, out=out)}, a.reps)
    rate = 16 * N / med(t["copy"])
    frac = lambda key, B: f"  {B:3d} B/cell -> {B * N / med(t[key]) / 1e9:6.3f} TB/s = {B * N / med(t[key]) / rate:6.1%} of the copy rate"
    lines.append(line("device-to-device copy of one field", t["copy"], frac("copy", 16)))
    lines.append(line("one Chebyshev step (k_scalar_cheb<0>)", t["cheb"], frac("cheb", 40)))
    lines.append(line("the first Chebyshev step (k_scalar_cheb<1>, no d read)", t["first"], frac("first", 32)))
    lines.append(line("fl_scalar_diffusion_apply (k_scalar_cheb<2>)", t["apply"], frac("apply", 16)))
    lines.append(line("one stage (fl_scalar_rhs, k_scalar_stage superbee)", t["stage"], frac("stage", 40)))
    lines.append(f"  Chebyshev step / stage = {med(t['cheb']) / med(t['stage']):.3f}")

    # ---- whole steps
    dt = 0.2 / n
    lines.append(f"one step over dt = {dt:g}: IMEX (theta = 1, rtol 1e-6, 5 explicit stages) beside the explicit step with the fewest stable stages")
    for number in a.numbers:
        gamma = number / (dt * 6.0 * h2)
        S.set_diffusivity(gamma)
        cfl = S.cfl(dt)
        stages = int(math.ceil(cfl[1])) + 1
        work = phi.clone()
        info = {}

        def imex():
            work.copy_(phi)
            info.update(S.step_imex(work, dt, 5, 1.0, 1e-6, 100000))

        def explicit():
            work.copy_(phi)
            S.step(work, dt, stages)
        t = alternating({"imex": imex, "explicit": explicit, "copy": lambda: work.copy_(phi)}, max(3, a.reps // 2), warm=1)
        cp = med(t["copy"])
        lines.append(f"  out[1] = {cfl[1]:.3f} (convective {cfl[0]:.3f}): {info['steps']} Chebyshev steps (B_k = {info['bound']:.2e}); explicit: {stages} stages;"
                     f" both timed with a copy of phi in front ({cp:.4f} ms, subtracted below)")
        lines.append(line(f"    IMEX step, {info['steps']} + 5 launches", [x - cp for x in t["imex"]]))
        lines.append(line(f"    explicit step, {stages} launches", [x - cp for x in t["explicit"]]))
        lines.append(f"    IMEX / explicit = {(med(t['imex']) - cp) / (med(t['explicit']) - cp):.3f}")
        del work
    S.close()
    P.close()
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
