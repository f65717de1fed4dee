"""An arena of caller arrays: what a foreign caller of the C-ABI hands in -- sub-vectors of one allocation that are 8-byte aligned and no better,
with somebody else's data right behind them -- instead of arrays that are each their own torch allocation (256-byte aligned, followed by slack).

Arena(spec, placement, device) makes ONE 1-D fp64 tensor and contiguous views into it, spec = [(name, length, role)], role "in" / "out" / "inout":

  A  the control: every array on a 16-byte boundary, at least GUARD guard doubles before, between and after the arrays
  B  every array 8 bytes off a 16-byte boundary, guards as in A
  C  the phases alternate with the array's index in spec (0, 8, 0, 8, ... bytes), guards as in A
  D  packed: the arrays back to back in spec order with nothing between them, GUARD doubles at both ends, the first array 8 bytes off; an odd
     length flips the phase of everything behind it, as in a nest vector

Guards beside an array that is written hold SENTINEL, a finite number of order one with a recognisable bit pattern: a stray `+= x` changes it (it
would leave the bits of a NaN, and of a huge number, as they are).  Guards that touch only "in" arrays hold NaN: a stray read that reaches a result
shows there.  "out" arrays start as SENTINEL.  After the caller has filled the inputs, freeze() keeps a copy of every word; check(written=...)
compares on int64 views: every guard word, every "in" array and every array not named in `written` is unchanged, and every "out" array that is
named lost its sentinel in every entry (all but those in `partial`)."""
import numpy as np
import torch

GUARD = 64
SENTINEL_BITS = 0x3FF5A5A5A5A5A5A5
SENTINEL = float(np.array([SENTINEL_BITS], dtype=np.int64).view(np.float64)[0])       # 1.3529...
PLACEMENTS = ("A", "B", "C", "D")
ROLES = ("in", "out", "inout")


class ArenaError(AssertionError):
    """array: the array whose neighbourhood (or content) changed; where: "before" its start, "after" its end or "inside"; offset: the first changed
    word, counted from 1 away from the array ("before" / "after") or from 0 inside it"""

    def __init__(self, msg, array, where, offset):
        super().__init__(msg)
        self.array, self.where, self.offset = array, where, offset


def layout(spec, placement, flip=()):
    """-> (starts in doubles from a 16-byte aligned base, total length).  flip: names that take the other phase than the placement gives (A - C)"""
    assert placement in PLACEMENTS, placement
    starts, pos = [], GUARD
    for i, (name, length, role) in enumerate(spec):
        assert role in ROLES and length >= 0, (name, length, role)
        if placement == "D":
            if i == 0:
                pos += 1
        else:
            odd = {"A": 0, "B": 1, "C": i % 2}[placement] ^ (1 if name in flip else 0)
            pos += (pos + odd) % 2
        starts.append(pos)
        pos += length + (0 if placement == "D" else GUARD)
    assert placement != "D" or not flip
    return starts, pos + (GUARD if placement == "D" else 0)


class Arena:
    def __init__(self, spec, placement, device="cuda", flip=()):
        self.spec = [(str(n), int(l), str(r)) for n, l, r in spec]
        self.names = [n for n, _, _ in self.spec]
        assert len(set(self.names)) == len(self.names), "array names must differ"
        self.placement, self.device = placement, device
        self.starts, self.total = layout(self.spec, placement, flip)
        self.length = {n: l for n, l, _ in self.spec}
        self.role = {n: r for n, _, r in self.spec}
        self.start = dict(zip(self.names, self.starts))
        raw = torch.empty(self.total + 1, dtype=torch.float64, device=device)
        self.buf = raw[(raw.data_ptr() // 8) % 2:][:self.total]
        assert self.buf.data_ptr() % 16 == 0, "the arena's base is not 16-byte aligned"
        # what every word is: -1 a guard, else the index of the array that owns it
        self.owner = np.full(self.total, -1, dtype=np.int64)
        for i, (n, l, r) in enumerate(self.spec):
            assert (self.owner[self.starts[i]:self.starts[i] + l] == -1).all()
            self.owner[self.starts[i]:self.starts[i] + l] = i
        fill = np.full(self.total, np.nan)
        edges = [0] + [e for s, (n, l, r) in zip(self.starts, self.spec) for e in (s, s + l)] + [self.total]
        for k in range(len(self.spec) + 1):                 # the guard before array k (after array k - 1)
            lo, hi = edges[2 * k], edges[2 * k + 1]
            beside = [self.spec[j][2] for j in (k - 1, k) if 0 <= j < len(self.spec)]
            if any(r != "in" for r in beside):
                fill[lo:hi] = SENTINEL
        for s, (n, l, r) in zip(self.starts, self.spec):
            fill[s:s + l] = SENTINEL if r == "out" else 0.0
        self.buf.copy_(torch.from_numpy(fill))
        self.views = {n: self.buf[s:s + l] for s, (n, l, r) in zip(self.starts, self.spec)}
        for i, (n, l, r) in enumerate(self.spec):
            v = self.views[n]
            assert v.is_contiguous() and v.numel() == l and v.data_ptr() == self.buf.data_ptr() + 8 * self.starts[i]
            assert v.data_ptr() % 16 == self.expected_phase(i, flip), (placement, n, v.data_ptr() % 16)
        self.frozen = None

    def expected_phase(self, i, flip=()):
        """the placement's statement of data_ptr() % 16 for array i, restated apart from layout()"""
        if self.placement == "D":
            return 8 * ((1 + sum(l for _, l, _ in self.spec[:i])) % 2)
        odd = {"A": 0, "B": 1, "C": i % 2}[self.placement]
        return 8 * (odd ^ (1 if self.names[i] in flip else 0))

    def __getitem__(self, name):
        return self.views[name]

    def phase(self, name):
        return self.views[name].data_ptr() % 16

    def phases(self):
        return {n: self.phase(n) for n in self.names}

    def fill(self, name, values):
        assert self.role[name] != "out", f"{name} is an output: it starts as the sentinel"
        a = np.ascontiguousarray(values, dtype=np.float64).reshape(-1)
        assert a.size == self.length[name], (name, a.size, self.length[name])
        self.views[name].copy_(torch.from_numpy(a))
        return self.views[name]

    def freeze(self):
        """keep every word as it is now: the state check() compares with"""
        self.frozen = self.words()
        return self

    def words(self):
        if self.buf.is_cuda:
            torch.cuda.synchronize()
        return self.buf.cpu().numpy().view(np.int64).copy()

    def get(self, name):
        """host copy of an array"""
        s = self.start[name]
        return self.words()[s:s + self.length[name]].view(np.float64).copy()

    def _describe(self, q):
        """the word q of the arena in terms of the arrays: (array, where, offset, text)"""
        i = int(self.owner[q])
        if i >= 0:
            n, off = self.names[i], q - self.starts[i]
            text = f"word {off} of {n!r} ({self.role[n]}, {self.length[n]} long)"
            if off == 0 and i > 0 and self.starts[i - 1] + self.spec[i - 1][1] == q:
                text += f", the word right behind the end of {self.names[i - 1]!r}"
            return n, "inside", off, text
        ends = [(q - (s + l) + 1, n) for s, (n, l, r) in zip(self.starts, self.spec) if s + l <= q]
        begs = [(s - q, n) for s, (n, l, r) in zip(self.starts, self.spec) if s > q]
        after, before = (min(ends) if ends else None), (min(begs) if begs else None)
        if before is None or (after is not None and after[0] <= before[0]):
            return after[1], "after", after[0], f"guard word {after[0]} past the end of {after[1]!r}"
        return before[1], "before", before[0], f"guard word {before[0]} before the start of {before[1]!r}"

    def check(self, written=(), partial=()):
        assert self.frozen is not None, "freeze() the arena once the inputs are in"
        written, partial = set(written), set(partial)
        for n in written | partial:
            assert n in self.role and self.role[n] != "in", f"{n}: not an array this call may write"
        now = self.words()
        may = np.zeros(self.total, dtype=bool)
        for i, n in enumerate(self.names):
            if n in written:
                may[self.starts[i]:self.starts[i] + self.length[n]] = True
        bad = np.flatnonzero((now != self.frozen) & ~may)
        if bad.size:
            q = int(bad[0])
            array, where, offset, text = self._describe(q)
            raise ArenaError(f"placement {self.placement}: {text} changed from {self.frozen[q:q + 1].view(np.float64)[0]!r} to "
                             f"{now[q:q + 1].view(np.float64)[0]!r} ({bad.size} words changed outside {sorted(written)})", array, where, offset)
        for i, n in enumerate(self.names):
            if n in written and self.role[n] == "out" and n not in partial:
                left = np.flatnonzero(now[self.starts[i]:self.starts[i] + self.length[n]] == SENTINEL_BITS)
                if left.size:
                    raise ArenaError(f"placement {self.placement}: word {int(left[0])} of {n!r} (out) still holds the sentinel "
                                     f"({left.size} of {self.length[n]} entries were not written)", n, "inside", int(left[0]))
