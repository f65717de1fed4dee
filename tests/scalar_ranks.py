"""What the several-rank passive-scalar tests share (tests/test_scalar_ranks_host.py, tests/test_gpu_scalar_ranks*.py): the case object the
handle helpers of tests/test_gpu_config5.py take (_handle, _blk, _fblk), scatter of global fields to the ranks' blocks and gather of the blocks,
and the geometry count of the wire -- numpy only, no GPU, no library."""
import numpy as np

from tests import scalar_cases as sc
from tests import scalar_reference as sr


class Case:
    """A grid of tests/scalar_cases.py on a rank grid.  own: cells per rank along each axis (None: DMStag's default split, larger blocks first)."""

    def __init__(self, n, ranks, bcname, uniform=True, own=None, kappa=1e-3):
        self.n, self.ranks, self.bcname, self.uniform, self.kappa = tuple(n), tuple(ranks), bcname, uniform, kappa
        self.kinds, self.vals = sc.BC_SETS[bcname]
        self.own = own if own is not None else [default_split(n[d], ranks[d]) for d in range(3)]
        assert all(sum(self.own[d]) == n[d] and len(self.own[d]) == ranks[d] for d in range(3))
        self.xf = sc.faces(self.n, uniform)
        self.periodic = [self.kinds[2 * d] == sr.PERIODIC for d in range(3)]
        self.bc = [3 if self.kinds[b] == sr.PERIODIC else 1 for b in range(6)]      # fl_bc: 1 velocity, 3 periodic (scalar_cases.poisson_bc)
        self.shp = (n[2], n[1], n[0])
        nf = [n[d] if self.periodic[d] else n[d] + 1 for d in range(3)]
        self.fshape = [(n[2], n[1], nf[0]), (n[2], nf[1], n[0]), (nf[2], n[1], n[0])]
        self.size = ranks[0] * ranks[1] * ranks[2]

    def problem(self):
        return sc.problem(self.n, self.uniform, self.bcname)

    def coord(self, rank):
        """x fastest, as DMStag numbers its ranks"""
        rx, ry, _ = self.ranks
        return (rank % rx, (rank // rx) % ry, rank // (rx * ry))

    def lo_len(self, rank):
        c = self.coord(rank)
        return [sum(self.own[d][:c[d]]) for d in range(3)], [self.own[d][c[d]] for d in range(3)]

    def cell_slices(self, rank):
        lo, ln = self.lo_len(rank)
        return tuple(slice(lo[a], lo[a] + ln[a]) for a in (2, 1, 0))

    def face_slices(self, rank, axis):
        """the faces a rank owns: those in front of its cells, and the last one of a non-periodic axis on its last rank (the layout of fl_poisson_rhs)"""
        lo, ln = self.lo_len(rank)
        c = self.coord(rank)
        sl = []
        for a in (2, 1, 0):
            m = ln[a] + (1 if a == axis and c[a] == self.ranks[a] - 1 and not self.periodic[a] else 0)
            sl.append(slice(lo[a], lo[a] + m))
        return tuple(sl)

    def neighbours(self, rank):
        """per boundary 2 d + side: whether a neighbouring rank sits behind it (an axis one rank holds alone has none: a periodic one wraps inside the block)"""
        c = self.coord(rank)
        out = []
        for d in range(3):
            r = self.ranks[d]
            out += [r > 1 and (c[d] > 0 or self.periodic[d]), r > 1 and (c[d] < r - 1 or self.periodic[d])]
        return out


def default_split(n, r):
    return tuple(n // r + (1 if a < n % r else 0) for a in range(r))


def scatter_cells(case, a):
    a = np.asarray(a).reshape(case.shp)
    return [np.ascontiguousarray(a[case.cell_slices(r)]) for r in range(case.size)]


def scatter_faces(case, a, axis):
    a = np.asarray(a).reshape(case.fshape[axis])
    return [np.ascontiguousarray(a[case.face_slices(r, axis)]) for r in range(case.size)]


def gather_cells(case, blocks):
    out = np.full(case.shp, np.nan)
    for r, b in enumerate(blocks):
        sl = case.cell_slices(r)
        out[sl] = np.asarray(b).reshape(out[sl].shape)
    assert not np.isnan(out).any()
    return out


def gather_faces(case, blocks, axis):
    out = np.full(case.fshape[axis], np.nan)
    for r, b in enumerate(blocks):
        sl = case.face_slices(r, axis)
        out[sl] = np.asarray(b).reshape(out[sl].shape)
    assert not np.isnan(out).any()
    return out


def plane(case, rank, d):
    _, ln = case.lo_len(rank)
    return ln[0] * ln[1] * ln[2] // ln[d]


def wire_phi(case, rank):
    """(messages, bytes) a rank sends in ONE exchange of phi: two planes of doubles across every boundary with a neighbouring rank"""
    nb = case.neighbours(rank)
    return sum(nb), sum(2 * 8 * plane(case, rank, b // 2) for b in range(6) if nb[b])


def wire_velocity(case, rank):
    """(messages, bytes) a rank sends in one exchange of the high faces of V: its first face plane to the rank behind its low end"""
    nb = case.neighbours(rank)
    return sum(nb[0::2]), sum(8 * plane(case, rank, d) for d in range(3) if nb[2 * d])


def wire_rhs(case, rank):
    return tuple(a + b for a, b in zip(wire_phi(case, rank), wire_velocity(case, rank)))


def wire_step(case, rank, s):
    (m, b), (mv, bv) = wire_phi(case, rank), wire_velocity(case, rank)
    return s * m + mv, s * b + bv


# the cases of tests/test_gpu_scalar_ranks.py (the host test scatters and gathers every one of them)
def rhs_cases():
    out = []
    for ranks in [(2, 1, 1), (1, 2, 1), (1, 1, 2)]:
        out.append(Case((4, 4, 4), ranks, "periodic"))
    for bcname in ("dirichlet", "periodic"):
        out.append(Case((6, 5, 4), (3, 1, 1), bcname, uniform=False))
        out.append(Case((4, 5, 6), (1, 1, 3), bcname, uniform=False))
    for bcname in sc.BC_SETS:
        for uniform in (True, False):
            out.append(Case((7, 5, 6), (2, 1, 1), bcname, uniform=uniform, own=[(5, 2), (5,), (6,)]))
        out.append(Case((7, 6, 5), (2, 2, 2), bcname, uniform=False))
    out.append(Case((7, 5, 6), (1, 2, 1), "channel", uniform=False))
    for ranks in [(2, 1, 1), (1, 2, 1), (1, 1, 2)]:
        out.append(Case((130, 6, 7), ranks, "channel", uniform=False))
    for bcname in ("channel", "periodic", "dirichlet"):
        out.append(Case((65, 64, 80), (1, 1, 2), bcname, uniform=False))
    return out


def case_id(c):
    return "x".join(map(str, c.n)) + "-" + "x".join(map(str, c.ranks)) + "-" + c.bcname + ("" if c.uniform else "-stretched")
