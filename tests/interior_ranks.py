"""Rank grids with INTERIOR ranks, named: three and four ranks per axis, so that a block has a neighbour on both sides of an axis and the two are
different ranks.  With two ranks on an axis every rank of a non-periodic axis touches a physical boundary and has one neighbour, and on a periodic
axis both faces go to the same peer: fl_halo_plan's general branch with two messages of one axis (fl_coeff.cpp), the send-only / receive-only pair
of fl_fill_hifaces to two different ranks, a block without wall rows whose local range does not start at a boundary (poisson_init), q stored for
two different peers (PlanA::qb), the a^-1 ring of k_schur_var_ring from two owners, ghost copies of owner-rank markers to -1 and +1 of one axis
and the per-block votes of three blocks are reached only here.

CASES names the grids, what each is there to reach and the marker sets of the IBM cases; tests/test_interior_ranks.py checks on the CPU that every
case really has such a rank and obeys the library's limits; tests/test_gpu_interior_ranks.py runs the flow solver on them over the in-process wire
(tests/inproc.py) against the single-domain oracle.  VOTE is the uneven split of the fused-smoother vote, SCHUR the cases that
tests/test_gpu_schur_var_multirank.py appends to its own; launch_regimes.RANK_REGIMES' ranks_std_z3 is the one interior block in an 8-wave plan."""
import numpy as np

V, O, PER, SYM = 1, 2, 3, 4
CAVITY = [V, V, V, V, SYM, V]
CHANNEL = [V, O, V, V, PER, PER]

# the library's own limits on a block (read from the code, not guessed)
IBM_OWNER_MIN = 4         # fl_ibm_owner.hip (routing of an owned set): a split axis with fewer than 4 cells on a rank is FL_ERR_ARG_OUTOFRANGE, voted
CHEB2_MIN = 2             # fl_cheb2.hip fl_cheb2_usable: at least 2 cells per axis for the fused two-step smoother
MG_MIN_EVEN = 8           # fl_mg.hip mg_build_levels: an axis is halved when every rank's range is even, starts even and has >= 8 cells


def _tanh_faces(n, lo, hi, beta):
    s = np.linspace(0.0, 1.0, n + 1)
    return lo + (hi - lo) * (np.tanh(beta * (2 * s - 1)) / np.tanh(beta) + 1) / 2


class InteriorCase:
    """A named rank grid.  Carries what the handle / block helpers of tests/test_gpu_config5.py (_handle, _blk, _fblk) and
    tests/test_gpu_schur_var_multirank.py (_session, _blocks) read from a case; the oracle grid and matrix are built on first use.
    stretched: the axes whose faces are clustered towards both ends (tanh, stronger along y and z as tests/gpu_common.py::stretched_faces)."""

    def __init__(self, name, n, ranks, own, bc, box, stretched, reaches, coarsens=False, kappa=1e-3):
        self.name, self.n, self.ranks, self.own, self.bc, self.box = name, tuple(n), tuple(ranks), own, list(bc), box
        self.stretched, self.reaches, self.coarsens, self.kappa = tuple(stretched), reaches, coarsens, kappa
        assert own is None or all(sum(own[d]) == n[d] and len(own[d]) == ranks[d] for d in range(3))
        self.size = ranks[0] * ranks[1] * ranks[2]
        self.xf = [_tanh_faces(n[d], box[d][0], box[d][1], 1.1 + 0.2 * d) if d in self.stretched else np.linspace(box[d][0], box[d][1], n[d] + 1)
                   for d in range(3)]
        self.nullspace = O not in bc
        self.periodic = [bc[0] == PER, bc[2] == PER, bc[4] == PER]
        self.shp = (n[2], n[1], n[0])
        self._g = self._S = None

    def __repr__(self):
        return f"{self.name} {self.n[0]}x{self.n[1]}x{self.n[2]} on {self.ranks[0]}x{self.ranks[1]}x{self.ranks[2]} ranks"

    def with_kappa(self, kappa):
        return InteriorCase(self.name, self.n, self.ranks, self.own, self.bc, self.box, self.stretched, self.reaches, self.coarsens, kappa)

    def on_ranks(self, ranks, own=None):
        """the same grid on another rank grid (the two-rank counterpart, the undecomposed grid)"""
        return InteriorCase(self.name, self.n, ranks, own, self.bc, self.box, self.stretched, self.reaches, self.coarsens, self.kappa)

    @property
    def g(self):
        if self._g is None:
            from oracle import fluca_oracle as fo
            self._g = fo.Grid(self.n, self.xf, self.bc, self.kappa)
        return self._g

    @property
    def S(self):
        if self._S is None:
            self._S = self.g.assemble_S()
        return self._S

    @property
    def fshape(self):
        n, g = self.n, self.g
        return [(n[2], n[1], g.nf[0]), (n[2], g.nf[1], n[0]), (g.nf[2], n[1], n[0])]

    def decomp(self, rank):
        """the fl_decomp of a rank: the default split, or the ownership ranges on the default rank grid (x fastest)"""
        from fluca_amd import capi
        from tests import mp_common as mpc
        return mpc.decomp_of(capi, self.n, self.ranks, rank, self.own)

    def blocks(self):
        """(nx, ny, nz) of every rank's block, in rank order"""
        return [tuple(int(self.decomp(r).len[a]) for a in range(3)) for r in range(self.size)]


CASES = [
    InteriorCase("x3_channel", (30, 12, 8), (3, 1, 1), None, CHANNEL, [(0.0, 3.0), (0.0, 1.2), (0.0, 0.8)], (1,),
                 "the inlet on rank 0, the outlet on rank 2, the middle block has neither; no null space; spacing 0.1 in x and z (markers)"),
    InteriorCase("y3_uneven", (12, 23, 9), (1, 3, 1), ([12], [8, 7, 8], [9]), [PER, PER, V, V, SYM, V], [(0.0, 1.0), (0.0, 1.0), (0.0, 0.5)], (0, 1, 2),
                 "an odd interior block between two even ones, a null space, x wraps inside the block; blocks of at most 8 rows: the momentum operator "
                 "reads whole stored fields (k_mom2)"),
    InteriorCase("x3_periodic", (21, 10, 8), (3, 1, 1), None, [PER] * 6, [(0.0, 1.0)] * 3, (),
                 "the smallest periodic axis on which every rank has two different peers; y and z coarsen, x (7 columns a rank) does not", coarsens=True),
    InteriorCase("z4_periodic", (16, 12, 20), (1, 1, 4), ([16], [12], [6, 4, 5, 5]), [V, V, V, V, PER, PER], [(0.0, 1.6), (0.0, 1.2), (0.0, 2.0)], (),
                 "two interior ranks, one of the smallest block owner-rank markers allow; the seam joins rank 3 to rank 0; spacing 0.1 (markers)"),
    InteriorCase("x3y2", (27, 16, 8), (3, 2, 1), None, CHANNEL, [(0.0, 2.7), (0.0, 1.6), (0.0, 0.8)], (),
                 "six ranks: the edge cells of the deep and the full exchange pass through an interior block in two hops; y and z coarsen, x does not", coarsens=True),
    InteriorCase("z3_mg", (16, 16, 48), (1, 1, 3), ([16], [16], [16, 16, 16]), CAVITY, [(0.0, 1.0), (0.0, 1.0), (0.0, 3.0)], (),
                 "even blocks of 16 cells: one coarsening, the tri-linear prolongation reaches across both rank faces of the middle block", coarsens=True),
]
BY_NAME = {c.name: c for c in CASES}

# which part of tests/test_gpu_interior_ranks.py runs on which case
OPERATOR = ["x3_channel", "y3_uneven", "x3_periodic", "z4_periodic", "x3y2"]
SMOOTHER = ["x3_periodic", "x3y2", "z3_mg"]          # all three with two multigrid levels
MOMENTUM = ["x3_channel", "y3_uneven", "z4_periodic"]
IBM = ["x3_channel", "z4_periodic"]

# the vote on the fused smoother over three uneven blocks: exactly the middle one is below fl_cheb2_agree's threshold (32 x 32 x 31 = 31744 cells
# between two blocks of 32768).  95 planes and not 94: an odd plane count is coarsened neither by the library (n % (2 ranks) != 0) nor by MgOracle
# (n odd), so the multigrid part of the smoother worker has one hierarchy to compare; with 94 MgOracle would halve z and the library would not.
VOTE = InteriorCase("z3_vote", (32, 32, 95), (1, 1, 3), ([32], [32], [32, 31, 32]), [V, V, V, V, PER, PER], [(0.0, 1.0), (0.0, 1.0), (0.0, 3.0)], (),
                    "the fuse decision is one decision of three ranks", coarsens=False)

# (n, rank grid, ownership ranges, boundary types) appended to tests/test_gpu_schur_var_multirank.py::CASES: three ranks on each axis in turn,
# uneven blocks of 3 - 8 cells, every x block a single tile (under 128 columns)
SCHUR = [
    ((17, 9, 8), (3, 1, 1), ([5, 8, 4], [9], [8]), [V, O, SYM, V, PER, PER]),           # x: a wall on rank 0, the outlet on rank 2
    ((9, 16, 7), (1, 3, 1), ([9], [6, 3, 7], [7]), [PER, PER, V, O, SYM, V]),           # y: a middle block of 3 rows -- its whole block is ring for somebody
    ((10, 9, 15), (1, 1, 3), ([10], [9], [4, 6, 5]), [O, V, SYM, O, PER, PER]),         # z periodic: three different peers round the seam
]


# ---------------------------------------------------------------------------------------------------------------- the plan, in numpy terms

def neighbours(case, rank):
    """(lo, hi) rank per axis of `rank`, by fl_decomp_neighbor"""
    from fluca_amd import capi
    import ctypes as C
    d = case.decomp(rank)
    per = (C.c_int * 3)(*[int(p) for p in case.periodic])
    return [(capi.lib.fl_decomp_neighbor(C.byref(d), per, 2 * a), capi.lib.fl_decomp_neighbor(C.byref(d), per, 2 * a + 1)) for a in range(3)]


def interior_axes(case, rank):
    """the axes on which `rank` has a low and a high neighbour that are two different ranks"""
    return [a for a, (lo, hi) in enumerate(neighbours(case, rank)) if lo >= 0 and hi >= 0 and lo != hi]


def halo_plan(case, rank):
    from fluca_amd import capi
    from tests import mp_common as mpc
    return mpc.halo_plan(capi, case.decomp(rank), case.periodic)


# ---------------------------------------------------------------------------------------------------------------- marker sets of the IBM cases

def _fibonacci_sphere(centre, radius, count):
    k = np.arange(count) + 0.5
    phi = np.arccos(1.0 - 2.0 * k / count)
    th = np.pi * (1.0 + 5.0 ** 0.5) * k
    return [centre[0] + radius * np.cos(th) * np.sin(phi), centre[1] + radius * np.sin(th) * np.sin(phi), centre[2] + radius * np.cos(phi)]


def spacing(case):
    """the uniform spacing of the split axis of an IBM case"""
    a = int(np.argmax(case.ranks))
    return (case.box[a][1] - case.box[a][0]) / case.n[a]


def markers(name):
    """The body of an IBM case: its supports straddle BOTH faces of the middle block along the split axis (tests/test_interior_ranks.py asserts it).
    x3_channel: an elliptic cylinder along the periodic span round the middle of the middle block (x = 1.0 .. 2.0), half-axes 5.5 cells in x and
    3.5 cells in y: it reaches half a cell into the blocks of rank 0 and rank 2, which own its two ends, and stays clear of the walls in y.
    z4_periodic: a sphere of radius 3.5 cells round the middle of rank 1's block of four planes (z = 0.6 .. 1.0), so
    that ranks 0 and 2 own caps of it, and a small cloud on the seam between rank 3 and rank 0 (z taken modulo the span)."""
    case = BY_NAME[name]
    h = spacing(case)
    if name == "x3_channel":
        a, b = 5.5 * h, 3.5 * h
        nth = int(round(np.pi * (a + b) / h))
        th = (np.arange(nth) + 0.5) * 2 * np.pi / nth
        zs = case.box[2][0] + (np.arange(case.n[2]) + 0.25) * h
        X = [np.concatenate([1.5 + a * np.cos(th) for _ in zs]), np.concatenate([0.6 + b * np.sin(th) for _ in zs]), np.repeat(zs, nth)]
    elif name == "z4_periodic":
        X = _fibonacci_sphere((0.8, 0.6, 0.8), 3.5 * h, 154)
        rng = np.random.default_rng(23)
        cl = rng.uniform(-2.5 * h, 2.5 * h, (3, 60)) + np.array([0.8, 0.6, 0.0])[:, None]
        cl[2] %= case.box[2][1]
        X = [np.concatenate([a, b]) for a, b in zip(X, cl)]
    else:
        raise KeyError(name)
    return [np.ascontiguousarray(a) for a in X]


def migration_path(name):
    """Positions before and after two calls of fl_ibm_migrate, per marker, along the split axis of an IBM case (spacing h, the middle block B of
    rank 1, its low face at a, its high face at b):
      call 1: the markers of B within a cell of a leave to rank 0, those within a cell of b leave to rank 2, while markers of rank 0 and of rank 2
              next to B arrive -- leavers in both directions and arrivals from both sides in one call; the `runner` goes from rank 0 into B;
      call 2: the runner goes on from B to rank 2, everything else drifts by a fifth of a cell.
    -> (path, runner): path[k] = [x, y, z] at call k (path[0]: creation), runner = index of the marker that passes 0 -> 1 -> 2."""
    case = BY_NAME[name]
    h = spacing(case)
    ax = int(np.argmax(case.ranks))
    own = case.own[ax] if case.own is not None else [case.n[ax] // case.ranks[ax]] * case.ranks[ax]
    a, b = case.box[ax][0] + own[0] * h, case.box[ax][0] + (own[0] + own[1]) * h
    other = [d for d in range(3) if d != ax]
    rng = np.random.default_rng(31)
    groups = [  # (count, position along the split axis before, after call 1)
        (12, a + rng.uniform(0.1, 0.9, 12) * h, lambda s: s - 1.1 * h),      # B -> rank 0
        (12, b - rng.uniform(0.1, 0.9, 12) * h, lambda s: s + 1.1 * h),      # B -> rank 2
        (10, a - rng.uniform(0.1, 0.9, 10) * h, lambda s: s + 1.1 * h),      # rank 0 -> B
        (10, b + rng.uniform(0.1, 0.9, 10) * h, lambda s: s - 1.1 * h),      # rank 2 -> B
        (16, rng.uniform(a + 1.2 * h, b - 1.2 * h, 16), lambda s: s + 0.1 * h),   # stay in B
        (1, np.array([a - 0.4 * h]), lambda s: s + 0.9 * h),                 # the runner: rank 0 -> B
    ]
    s0 = np.concatenate([g[1] for g in groups])
    s1 = np.concatenate([g[2](g[1]) for g in groups])
    L = s0.size
    runner = L - 1
    s2 = s1 + 0.2 * h
    s2[runner] = b + 0.4 * h                                                 # ... and on to rank 2, right across B
    mid = [0.5 * (case.box[d][0] + case.box[d][1]) for d in other]
    t = [mid[k] + rng.uniform(-2.0 * h, 2.0 * h, L) for k in range(2)]
    path = []
    for s in (s0, s1, s2):
        X = [None] * 3
        X[ax], X[other[0]], X[other[1]] = s, t[0], t[1]
        path.append([np.ascontiguousarray(v) for v in X])
    return path, runner
