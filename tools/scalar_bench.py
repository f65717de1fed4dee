"""Time the passive-scalar stage kernel (fl_scalar.hip): one stage (fl_scalar_rhs: 40 B/cell compulsory) and one five-stage step (fl_scalar_step:
4 x 40 + 48 B/cell) at N^3 with HIP events -- inputs resident, warm-up, the spread over the repeats -- and, in the same process, the box's own
copy rate (a device-to-device copy of one field: 16 B/cell) and the fl_abf_schur_apply call with schurainv = DIAG, whose k_schur_var is the
project's other no-LDS kernel with a five-cell window.  Counter bytes (FETCH_SIZE, WRITE_SIZE) and kernel durations come from rocprofv3 runs of
their own over this script (--only-scalar keeps them short); profiles/README.md has the command lines.

--ring: k_scalar_stage_ring beside k_scalar_stage on the same 512 x 512 x 256 block, in the same process: rank 0 of a 1 x 1 x 2 grid (two handles, two
threads, the in-memory transport of tests/inproc.py) makes one collective fl_scalar_rhs, then times the launch ALONE (fldbg_scalar_stage_only: no
exchange) while its peer idles; the one-rank kernel on a one-rank handle of the block's size is timed twice around it -- the spread of those two runs is
the noise floor.  No pass / fail number: profiles/scalar_ranks.txt.

usage: python tools/scalar_bench.py [--cells 256 512] [--reps 20] [--limiter superbee] [--only-scalar] [--ring] [--out FILE]"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch

from fluca_amd.poisson import Momentum, Poisson
from fluca_amd.scalar import DIRICHLET, NEUMANN, PERIODIC, Scalar
from oracle import fluca_oracle as fo


def timed(fn, reps, warm=3):
    """-> sorted times in ms of `reps` calls, each bracketed by HIP events on the current stream"""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return sorted(out)


def line(what, ms, bytes_per_cell, ncell, extra=""):
    med = statistics.median(ms)
    return f"  {what:<44s} median {med:8.4f} ms  (min {ms[0]:.4f}, max {ms[-1]:.4f}, {len(ms)} repeats)  {bytes_per_cell:4d} B/cell compulsory -> {bytes_per_cell * ncell / med / 1e9:7.3f} TB/s{extra}"


RING_BLOCK = (512, 512, 256)
RING_BC = (DIRICHLET, NEUMANN, NEUMANN, NEUMANN, NEUMANN, NEUMANN)     # (z is split: a kind behind a rank face is accepted and unused)


def _fields(P, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    rnd = lambda m: torch.rand(m, dtype=torch.float64, device="cuda", generator=g) - 0.5
    return [rnd(P.nface[d]) for d in range(3)], rnd(P.ncell) + 0.5, torch.empty(P.ncell, dtype=torch.float64, device="cuda")


def _ring_rank(R, limiter, reps, result):
    """one rank of the 1 x 1 x 2 grid: both make the handle and one collective call; rank 0 then times the launch alone"""
    import ctypes as C

    from fluca_amd import capi
    from tests import mp_common as mpc
    nx, ny, nz = RING_BLOCK
    n = (nx, ny, 2 * nz)
    xf = [np.linspace(0.0, 1.0, m + 1) for m in n]
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    P = Poisson(n, xf, [fo.BC_VELOCITY] * 6, 1e-3, decomp=mpc.decomp_of(capi, n, (1, 1, 2), R.rank))
    P.set_stream(stream)
    R.attach(P.h)
    S = Scalar(P, RING_BC, (1.0, 0.0, 0.0, 0.0, 0.0, 0.0), limiter=limiter, gamma=1e-3)
    V, phi, out = _fields(P, 3 + R.rank)
    S.set_velocity(*V)
    S.rhs(phi, out=out)                   # collective: the slabs and the high faces of V arrive
    stream.synchronize()
    R.barrier()
    if R.rank == 0:
        f = capi.lib.fldbg_scalar_stage_only
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        ptr = lambda t: C.c_void_p(t.data_ptr())
        for pack in (0, 1):
            def launch():
                capi.check(f(S.h, ptr(phi), None, ptr(out), pack), "fldbg_scalar_stage_only")
            result[pack] = timed(launch, reps)
    R.barrier()                           # (the peer idles until rank 0 is done)
    S.close()
    P.close()


def ring_leg(a, lines):
    from tests import inproc
    nx, ny, nz = RING_BLOCK
    N = nx * ny * nz
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)

    def one_rank():
        xf = [np.linspace(0.0, 1.0, nx + 1), np.linspace(0.0, 1.0, ny + 1), np.linspace(0.0, 0.5, nz + 1)]
        P = Poisson(RING_BLOCK, xf, [fo.BC_VELOCITY] * 6, 1e-3)
        P.set_stream(stream)
        S = Scalar(P, RING_BC, (1.0, 0.0, 0.0, 0.0, 0.0, 0.0), limiter=a.limiter, gamma=1e-3)
        V, phi, out = _fields(P, 3)
        S.set_velocity(*V)
        ms = timed(lambda: S.rhs(phi, out=out), a.reps)
        S.close()
        P.close()
        return ms
    first = one_rank()
    torch.cuda.empty_cache()
    result = {}
    inproc.run_threads(2, _ring_rank, a.limiter, a.reps, result)
    torch.cuda.empty_cache()
    torch.cuda.set_stream(stream)
    second = one_rank()
    m1, m2, r0, r1 = (statistics.median(x) for x in (first, second, result[0], result[1]))
    base = 0.5 * (m1 + m2)
    lines.append(f"--ring: one stage on a {nx} x {ny} x {nz} block ({N * 8 / 2 ** 30:.2f} GiB a field), limiter {a.limiter}, Gamma 1e-3, random V and phi, HIP events around the launch")
    lines.append(line("k_scalar_stage (one rank), first run", first, 40, N))
    lines.append(line("k_scalar_stage (one rank), second run", second, 40, N))
    lines.append(f"  noise floor: the two runs' medians differ by {abs(m1 - m2):.4f} ms = {abs(m1 - m2) / base:.2%} of their mean {base:.4f} ms")
    lines.append(line("k_scalar_stage_ring, rank 0 of 1 x 1 x 2", result[0], 40, N))
    lines.append(line("k_scalar_stage_ring with the fused pack", result[1], 40, N))
    lines.append(f"  ring / one rank = {r0 / base:.4f}; with the fused pack = {r1 / base:.4f}  (the ring block has a rank face at its high z end: one z slab read, two layers packed)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--limiter", default="superbee")
    ap.add_argument("--only-scalar", action="store_true")
    ap.add_argument("--ring", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "scalar_bench.py needs a GPU"
    # one stream of its own for the library's kernels, torch's copies and the events that bracket them (the null stream would send the library
    # back to the handle's own stream, and the events would time nothing)
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    what = "--ring" if a.ring else f"--cells {' '.join(map(str, a.cells))}" + (" --only-scalar" if a.only_scalar else "")
    lines = [f"tools/scalar_bench.py {what} --reps {a.reps} --limiter {a.limiter}   ({torch.cuda.get_device_name(0)})"]
    if a.ring:
        ring_leg(a, lines)
        a.cells = []
    for n in a.cells:
        V_, PER = fo.BC_VELOCITY, fo.BC_PERIODIC
        xf = [np.linspace(0.0, 1.0, n + 1) for _ in range(3)]
        P = Poisson((n, n, n), xf, [V_, V_, V_, V_, PER, PER], 1e-3)
        P.set_stream(stream)
        N = n ** 3
        g = torch.Generator(device="cuda").manual_seed(3)
        rnd = lambda m: torch.rand(m, dtype=torch.float64, device="cuda", generator=g) - 0.5
        # a channel: Dirichlet x-, Neumann 0 at x+, Neumann in y, periodic z
        S = Scalar(P, (DIRICHLET, NEUMANN, NEUMANN, NEUMANN, PERIODIC, PERIODIC), (1.0, 0.0, 0.0, 0.0, 0.0, 0.0), limiter=a.limiter, gamma=1e-3)
        V = [rnd(P.nface[d]) for d in range(3)]
        S.set_velocity(*V)
        phi, out = rnd(N) + 0.5, torch.empty(N, dtype=torch.float64, device="cuda")
        dt = 0.2 / n
        lines.append(f"{n}^3 cells ({N * 8 / 2 ** 30:.2f} GiB a field), limiter {a.limiter}, Gamma 1e-3, random V and phi")
        if not a.only_scalar:
            copy = timed(lambda: out.copy_(phi), a.reps)
            lines.append(line("device-to-device copy of one field", copy, 16, N))
        stage = timed(lambda: S.rhs(phi, out=out), a.reps)
        step = timed(lambda: S.step(phi, dt, 5), a.reps)
        if a.only_scalar:
            lines.append(line("one stage (fl_scalar_rhs)", stage, 40, N))
            lines.append(line("one five-stage step (fl_scalar_step)", step, 208, N))
        else:
            rate = 16 * N / statistics.median(copy)
            frac = lambda ms, b: f"  = {b * N / statistics.median(ms) / rate:5.1%} of the copy rate"
            lines.append(line("one stage (fl_scalar_rhs)", stage, 40, N, frac(stage, 40)))
            lines.append(line("one five-stage step (fl_scalar_step)", step, 208, N, frac(step, 208)))
            M = Momentum(P)
            v0 = 8.0 * rnd(3 * N)
            M.set_state(1e-3, 1.0, 0.05, [8.0 * v for v in V], M.interp_faces(v0), v0=v0)
            M.set_ainv_types(schur=fo.AINV_DIAG)
            p = rnd(N)
            sv = timed(lambda: M.schur_apply(p), a.reps)
            lines.append(line("fl_abf_schur_apply, DIAG (k_schur_var + set-up)", sv, 40, N, f"  stage / this call = {statistics.median(stage) / statistics.median(sv):.3f}"))
            M.close()
        S.close()
        P.close()
        del V, phi, out
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
