"""No GPU: the harness of tests/test_gpu_handle_history.py (tests/handle_history.py) -- the walk is an Eulerian circuit, the shipped seeds and
catalogues meet the coverage condition, a backend whose results depend on the logical state alone passes, and three deliberately broken backends
are each reported with the operation, its predecessors and the state: the evidence that the GPU test would notice the bug class."""
import hashlib
from collections import Counter

import numpy as np
import pytest

from tests import handle_history as hh

CATALOGUES = {"one rank": (hh.catalogue, hh.SEEDS), "two ranks": (hh.rank_catalogue, (hh.RANK_SEED,))}
CASES = [(name, seed) for name, (_, seeds) in CATALOGUES.items() for seed in seeds]


def _ops(name):
    return CATALOGUES[name][0]()


def test_catalogue_is_well_formed():
    for name in CATALOGUES:
        ops = _ops(name)
        names = [o.name for o in ops]
        assert len(set(names)) == len(names)
        for o in ops:
            assert o.kind in ("query", "setter") and o.handle
            if o.kind == "setter":
                (var, val), = o.sets.items()
                assert val in hh.VARS[var]
            else:
                assert all(v in hh.VARS for v in o.proj)
                assert "stream" not in o.proj, "the stream is in no projection"
                assert ("knobs" not in o.proj) or o.why, f"{o.name}: say why the knob profile may change its arithmetic"
    # one rank: every variable has a setter for each of its values
    sets = Counter(v for o in _ops("one rank") if o.kind == "setter" for v in o.sets)
    assert sets == Counter({v: len(vals) for v, vals in hh.VARS.items()})


@pytest.mark.parametrize("name,seed", CASES)
def test_walk_is_an_eulerian_circuit_and_a_pure_function(name, seed):
    ops = _ops(name)
    k = len(ops)
    steps = hh.walk(ops, seed)
    assert len(steps) == k * k + 1 and steps[0] == steps[-1]
    pairs = Counter(zip(steps, steps[1:]))
    assert len(pairs) == k * k and set(pairs.values()) == {1}          # every ordered pair, loops included, exactly once
    assert {a for a, _ in pairs} == {o.name for o in ops}
    hh._WALKS.clear()                                                    # computed again, not remembered
    assert hh.walk(ops, seed) == steps
    assert hh.walk(ops, seed + 1) != steps


@pytest.mark.parametrize("name,seed", CASES)
def test_coverage_condition_holds_for_the_shipped_seeds(name, seed):
    """every (query, projection value) that occurs: at least 3 visits after at least 3 different predecessors; every query meets every value of
    each variable of its projection"""
    ops = _ops(name)
    steps = hh.walk(ops, seed)
    assert hh.coverage_problems(ops, steps) == []
    seen = hh.visits(ops, steps)
    assert {q for q, _ in seen} == {o.name for o in ops if o.kind == "query"}
    assert sum(len(v) for v in seen.values()) == sum(1 for s in steps if s in {q for q, _ in seen})
    # the trajectory is the state the setters before a step have left
    tr = hh.trajectory(ops, steps)
    by = {o.name: o for o in ops}
    assert tr[0] == hh.initial(ops) and len(tr) == len(steps)
    for i in range(1, len(steps)):
        want = dict(tr[i - 1])
        if by[steps[i - 1]].kind == "setter":
            want.update(by[steps[i - 1]].sets)
        assert tr[i] == want


def test_coverage_check_notices_a_thin_walk():
    ops = _ops("two ranks")
    steps = hh.walk(ops, hh.RANK_SEED)
    assert hh.coverage_problems(ops, steps[:len(steps) // 6])           # a sixth of the circuit cannot meet the condition


def test_first_difference():
    a = {"x": np.array([1.0, 0.0, np.nan]), "n": 3}
    assert hh.first_difference(a, {"x": np.array([1.0, 0.0, np.nan]), "n": 3}) is None          # the same bits, NaN included
    assert hh.first_difference(a, {"x": np.array([1.0, -0.0, np.nan]), "n": 3})[:2] == ("x", 1)   # -0.0 is another bit pattern
    assert hh.first_difference(a, {"x": np.array([1.0, 0.0, np.nan]), "n": 4}) == ("n", 0, 3, 4)
    assert hh.first_difference(a, {"x": np.array([1.0, 0.0]), "n": 3})[1] == -1
    assert hh.first_difference(a, {"x": a["x"]})[0] == "<the set of outputs>"
    near = {"x": np.array([1.0 + 2e-16, 0.0, np.nan]), "n": 3}
    assert hh.first_difference(a, near) is not None and hh.first_difference(a, near, (1e-12, 0.0)) is None


# ------------------------------------------------------------------------------------------------------------------ fake backends

class Fake:
    """every query returns a hash of (name, projection value): a library without history"""

    def __init__(self, ops):
        self.state = hh.initial(ops)

    def setter(self, op, state):
        assert state == self.state                  # the harness and the backend agree on the logical state
        self.state.update(op.sets)

    def value(self, *what):
        return np.frombuffer(hashlib.sha256(repr(what).encode()).digest(), dtype=np.uint64).copy()

    def query(self, op, state):
        assert state == self.state
        return {"out": self.value(op.name, hh.projection(op, self.state))}


class StaleCache(Fake):
    """1. a cache that one setter fails to invalidate: the Gershgorin radius survives fl_momentum_set_state without v0 (profile M1)"""

    def __init__(self, ops):
        super().__init__(ops)
        self.cache = None

    def setter(self, op, state):
        super().setter(op, state)
        if "mom0" in op.sets and op.sets["mom0"] != "M1":
            self.cache = None

    def query(self, op, state):
        if op.name != "m0.gershgorin":
            return super().query(op, state)
        if self.cache is None:
            self.cache = super().query(op, state)
        return self.cache


class DirtyBuffer(Fake):
    """2. a work buffer that one operation leaves dirty for one other: the multigrid solve for the 12-step CG"""

    def __init__(self, ops):
        super().__init__(ops)
        self.dirty = False

    def query(self, op, state):
        if op.name == "p.solve mg levels 0":
            self.dirty = True
        if op.name == "p.solve cg 12" and self.dirty:
            self.dirty = False
            return {"out": self.value(op.name, "dirty")}
        return super().query(op, state)


class StreamDependent(Fake):
    """3. a result that depends on the stream variable"""

    def query(self, op, state):
        if op.name == "s0.rhs":
            return {"out": self.value(op.name, hh.projection(op, self.state), self.state["stream"])}
        return super().query(op, state)


@pytest.mark.parametrize("name,seed", CASES)
def test_a_backend_without_history_is_clean(name, seed):
    ops = _ops(name)
    assert hh.run(Fake(ops), ops, hh.walk(ops, seed)) == []


@pytest.mark.parametrize("seed", hh.SEEDS)
def test_the_three_broken_backends_are_reported(seed):
    ops = hh.catalogue()
    steps = hh.walk(ops, seed)
    fresh = lambda cls: hh.seed_expected(lambda: cls(ops), ops, [steps], {})     # as the GPU test seeds its table: one fresh backend per entry

    found = hh.run(DirtyBuffer(ops), ops, steps, fresh(DirtyBuffer))
    assert found and {f.op for f in found} == {"p.solve cg 12"}
    by = {o.name: o for o in ops}
    # the culprit right before it is among the reports (every ordered pair is in the walk), named as a predecessor
    direct = [f for f in found if f.predecessors[-1] == "p.solve mg levels 0"]
    assert len(direct) == 1 and "p.solve mg levels 0" in hh.describe(direct[0])
    for f in found:     # ... and in every report the culprit ran since the victim's last visit
        back = steps[:f.step][::-1]
        since = back[:back.index("p.solve cg 12")] if "p.solve cg 12" in back else back
        assert "p.solve mg levels 0" in since
    assert by["p.solve cg 12"].proj == ()

    found = hh.run(StreamDependent(ops), ops, steps, fresh(StreamDependent))
    assert found and {f.op for f in found} == {"s0.rhs"}
    assert {f.state["stream"] for f in found} == {"second"} and "'stream': 'second'" in hh.describe(found[0])
    assert hh.run(StreamDependent(ops), ops, steps)                     # the walk alone shows this one as well


def test_two_rank_catalogue_reports_a_broken_backend_too():
    ops = hh.rank_catalogue()
    found = hh.run(StreamDependent(ops), ops, hh.walk(ops, hh.RANK_SEED))
    assert found and {f.op for f in found} == {"s0.rhs"}


def test_a_cache_that_a_setter_fails_to_invalidate_is_reported():
    """The first broken backend.  The stale value shows only where the radius was asked for between the last setter that does invalidate and the
    one that does not, and on a walk whose state moves seldom every visit of a projection value can be stale in the SAME way: the walk alone then
    compares like with like.  Hence the table of fresh results (hh.seed_expected), and hence two walks: what is asserted is that the pair the GPU
    test runs reports it, every report naming the operation, its predecessors and the state."""
    ops = hh.catalogue()
    found = []
    for seed in hh.SEEDS:
        steps = hh.walk(ops, seed)
        found += hh.run(StaleCache(ops), ops, steps, hh.seed_expected(lambda: StaleCache(ops), ops, [steps], {}))
    assert found and {f.op for f in found} == {"m0.gershgorin"}
    assert all(f.state["mom0"] == "M1" for f in found)                  # the state in which the stale value shows
    for f in found:
        text = hh.describe(f)
        assert "m0.gershgorin" in text and "'mom0': 'M1'" in text and all(p in text for p in f.predecessors) and 1 <= len(f.predecessors) <= 3
