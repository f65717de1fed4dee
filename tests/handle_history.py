"""Helper of tests/test_handle_history.py and tests/test_gpu_handle_history.py (numpy only, no GPU, no library): does the HISTORY of a handle
change a result?

The property: in the same logical state an entry point returns the same bits whatever was called on the handles before.  It needs no oracle.
A live set of handles (one fl_poisson, two fl_momentum and two fl_scalar on it, one fl_ibm) is driven through a closed walk that contains every
ordered pair of operations exactly once; the first result of a (query, projection value) is kept, every later one must equal it byte for byte.

  catalogue    the operations: QUERIES compute something, SETTERS change one variable of the logical state
  state model  VARS: a few variables with few values each.  A query's PROJECTION is the tuple of variables its result may depend on; the
               stream is in no projection (that a stream switch changes nothing is part of what is tested), the knob profile only in those
               of operations whose arithmetic it legitimately changes (each entry says why)
  walk         an Eulerian circuit of the complete directed graph with loops on the operations, the vertex order permuted by the seed, the
               edges taken in an order that serves the coverage condition (coverage_problems)
  run          drives a backend (the GPU handles, or the fakes of tests/test_handle_history.py) through a walk and reports every result that
               differs from the first one of its (query, projection value), or from the one seed_expected took from a fresh backend
"""
import random
from collections import namedtuple

import numpy as np

VARS = {
    "mom0": ("M1", "M2", "M3"),        # M1 set_state without v0; M2 set_state_v0; M3 set_state_v0 of other fields, then set_coefficients(1, dt / 2, cL)
    "mom1": ("M1", "M2", "M3"),
    "ainv0": ("II", "DD", "RI"),       # (schur, upper) of fl_abf_set_ainv_types: ID/ID, DIAG/DIAG, ROWSUM/ID
    "ainv1": ("II", "DD", "RI"),
    "sc0": ("S1", "S2", "S3"),         # S1 superbee, Gamma 0; S2 venkatakrishnan, Gamma 0.0125, one boundary value changed; S3 upwind, new velocity arrays
    "sc1": ("S1", "S2", "S3"),
    "knobs": ("default", "alt"),
    "ibm": ("A", "B"),                 # marker positions; B through fl_ibm_update
    "stream": ("own", "second"),
}
INITIAL = {v: vals[0] for v, vals in VARS.items()}

# The seeds of the walks tests/test_gpu_handle_history.py runs: chosen (by trying seeds in ascending order) so that the coverage condition holds for
# the catalogues below; tests/test_handle_history.py checks that it does.  A change of a catalogue may need other seeds.
SEEDS = (13, 175)
RANK_SEED = 9

# the knob profile "alt" (process-wide, fl_tuning_set); "default" puts back what the process started with
ALT_KNOBS = dict(cheb_fuse=2, cheb_zero3=0, mg_prolong=0, mg_coarse=0, mg_post_smooth=1, cg_xdepth=2, cg_xbatch=0, schur_var_fused=0)

Op = namedtuple("Op", "name kind handle proj sets why")


def _q(name, handle, proj=(), why=""):
    return Op(name, "query", handle, tuple(proj), None, why)


def _s(var, value, handle):
    return Op(f"set {var}={value}", "setter", handle, (), {var: value}, "")


FUSE = "cheb_fuse 2 runs two Chebyshev steps per sweep on this small grid (another association of the recurrence: 1e-13, tests/test_gpu_cheb2.py)"
MGK = ("mg_prolong, mg_coarse and mg_post_smooth change the preconditioner (another algorithm / summation order, include/fluca_hip.h); "
       "cheb_fuse and cheb_zero3 change the smoother's launches")
SVF = "schur_var_fused 0 forms the DIAG / ROWSUM product as a composition of seven kernels: another order of the same sums"
NOK = ("cg_xdepth and cg_xbatch are NOT in the projection of the CG solves: every depth and both batch modes give x and the residual norms bit for "
       "bit (tests/test_gpu_cg_xring.py, tests/test_gpu_cg_xflush.py)")


def _momentum_queries(i, which):
    m, pm, pa = f"m{i}", (f"mom{i}",), (f"mom{i}", f"ainv{i}", "knobs")
    full = [
        _q(f"{m}.apply", m, pm), _q(f"{m}.diagonal", m, pm), _q(f"{m}.rowsum", m, pm), _q(f"{m}.gershgorin", m, pm),
        _q(f"{m}.chebyshev_interval", m, pm),
        _q(f"{m}.solve bcgs", m, pm), _q(f"{m}.solve gmres5", m, pm), _q(f"{m}.solve chebyshev", m, pm), _q(f"{m}.solve chebyshev guess", m, pm),
        # T, B and the buoyancy term are the grid's: no state of the handle enters
        _q(f"{m}.face_interp", m), _q(f"{m}.interp_faces", m), _q(f"{m}.add_buoyancy", m),
        # fl_momentum_rhs forms v0 + c L v0 with the handle's operator kernel: k_mom3 where the state came with v0 (M2, M3), k_mom2 otherwise (M1),
        # which add the terms of a row in another order -- the value is the state's, the last bit is the kernel's (found by the first walks)
        _q(f"{m}.rhs", m, pm),
        _q(f"{m}.jacobian_mult", m, pm),
        _q(f"{m}.schur_apply", m, pa, SVF),
        _q(f"{m}.abf_apply", m, pa, SVF + "; its Schur solve is Jacobi-PCG or, with DIAG / ROWSUM, flexible GMRES on that product"),
    ]
    return [o for o in full if which is None or o.name.split(".", 1)[1] in which]


def _scalar_queries(i, which):
    s, ps = f"s{i}", (f"sc{i}",)
    full = [_q(f"{s}.rhs", s, ps), _q(f"{s}.rhs source", s, ps), _q(f"{s}.step 5", s, ps), _q(f"{s}.step 2", s, ps), _q(f"{s}.cfl", s, ps),
            _q(f"{s}.stats", s), _q(f"{s}.boundary_flux", s, ps)]          # stats: min, max and the volume-weighted sum of phi read no setting
    return [o for o in full if which is None or o.name.split(".", 1)[1] in which]


def _setters(variables):
    handle = {"mom": "m", "ainv": "m", "sc": "s"}
    out = []
    for v in variables:
        h = {"knobs": "process", "ibm": "ibm", "stream": "p"}.get(v) or handle[v[:-1]] + v[-1]
        out += [_s(v, val, h) for val in VARS[v]]
    return out


def catalogue():
    """One rank: every entry point that computes something.  The second Momentum and Scalar handle carry the queries that touch state they
    share with the first (the work vectors and sv_pack of the Poisson handle, the slabs and hiface)."""
    p = [
        _q("p.apply", "p"), _q("p.diagonal", "p"), _q("p.rhs", "p"), _q("p.project", "p"), _q("p.gst_bc", "p"), _q("p.pressure_update", "p"),
        _q("p.gershgorin", "p"),
        _q("p.solve cg 12", "p", (), NOK), _q("p.solve cg rtol", "p", (), NOK), _q("p.solve cg single reduction 12", "p", (), NOK),
        _q("p.solve bcgs 12", "p"),
        _q("p.solve chebyshev 12", "p", ("knobs",), FUSE),
        _q("p.solve mg levels 0", "p", ("knobs",), MGK), _q("p.solve mg levels 2 smooth 2", "p", ("knobs",), MGK),
        _q("p.solve mg levels 1", "p", ("knobs",), MGK),
        _q("p.solve cg 600 history then short", "p", (), NOK), _q("p.solve cg nan", "p"),
        _q("p.vec_lincomb", "p"), _q("p.vec_dot", "p"), _q("p.vec_mdot", "p"), _q("p.vec_maxpy", "p"),
    ]
    ops = p + _momentum_queries(0, None) + _momentum_queries(1, {"apply", "chebyshev_interval", "solve chebyshev", "schur_apply", "abf_apply"})
    ops += _scalar_queries(0, None) + _scalar_queries(1, {"rhs", "step 5"})
    ops += [_q("ibm.interp", "ibm", ("ibm",)), _q("ibm.spread", "ibm", ("ibm",)), _q("ibm.force", "ibm", ("ibm",))]
    return ops + _setters(VARS)


def rank_catalogue():
    """Two ranks: what is rank-specific -- ghost layers, deep ghosts and xcap, the ring of a^-1, hiface and the slabs, the replicated markers'
    all-reduce.  One Momentum and one Scalar handle; the ainv profile without ROWSUM (the same kernel as DIAG on another vector)."""
    ops = [
        _q("p.solve cg 12", "p", (), NOK), _q("p.solve cg single reduction 12", "p", (), NOK),
        _q("p.solve chebyshev 12", "p", ("knobs",), FUSE), _q("p.solve mg levels 2 smooth 2", "p", ("knobs",), MGK),
        _q("p.rhs", "p"), _q("m0.apply", "m0", ("mom0",)), _q("m0.schur_apply", "m0", ("mom0", "ainv0", "knobs"), SVF),
    ]
    ops += _scalar_queries(0, {"rhs", "step 5", "cfl", "boundary_flux"}) + [_q("ibm.interp", "ibm")]
    sets = _setters(("mom0", "sc0", "knobs", "stream"))
    return ops + sets + [_s("ainv0", "II", "m0"), _s("ainv0", "DD", "m0")]


def initial(ops):
    """the default state of the variables the catalogue's setters move"""
    moved = {v for o in ops if o.kind == "setter" for v in o.sets} | {v for o in ops for v in o.proj}
    return {v: INITIAL[v] for v in VARS if v in moved}


def domain(ops):
    """variable -> the values it takes in this catalogue: the default and what the setters set"""
    out = {v: {val} for v, val in initial(ops).items()}
    for o in ops:
        if o.kind == "setter":
            for v, val in o.sets.items():
                out[v].add(val)
    return out


# ------------------------------------------------------------------------------------------------------------------ the walk

_WALKS = {}


def walk(ops, seed):
    """Names of the operations along a closed walk of k^2 steps (k^2 + 1 entries, the last is the first again): every ordered pair (A then B, A then A
    included) is one pair of neighbours exactly once -- an Eulerian circuit of the complete directed graph with loops.  A pure function of the
    catalogue and the seed.

    Construction: start at the root (the first vertex of the order the seed permutes) and always leave by an unused edge, the edge back to the
    root last of all edges of its vertex; such a walk ends at the root with every edge used (the edges to the root form a spanning in-tree: the
    "last exit" argument of the BEST theorem).  Within that rule the next edge is chosen for COVERAGE, by following the logical state along the
    walk: a query that has been met once or twice in its present projection value comes first, then anything that does not move the state (a
    query already met three times, a setter of the value that is set), then a query in a projection value that is new, and a setter that moves
    the state last -- so the state moves about as seldom as the k^2 edges allow (a setter right after another setter of the same variable must move
    it) and the visits of a (query, projection value) come in runs.  The seed's order breaks the ties."""
    key = (tuple((o.name, o.proj) for o in ops), seed)
    if key in _WALKS:
        return list(_WALKS[key])
    by = {o.name: o for o in ops}
    order = [o.name for o in ops]
    rng = random.Random(seed)
    rng.shuffle(order)
    root = order[0]
    unused = {a: list(order) for a in order}
    for a in order:
        rng.shuffle(unused[a])
    state, count = initial(ops), {}
    queries = [o for o in ops if o.kind == "query"]

    dom = domain(ops)
    values = {q.name: int(np.prod([len(dom[v]) for v in q.proj])) for q in queries}      # projection values a query can meet
    left = {q.name: len(order) for q in queries}                                        # visits it still has
    filled = {q.name: 0 for q in queries}                                               # projection values met three times
    started = {q.name: 0 for q in queries}                                              # ... met once or twice
    owed = {q.name: 0 for q in queries}                                                 # visits that complete the started ones
    started_keys = set()

    def score(w):
        op = by[w]
        if op.kind == "query":
            n = count.get((w, projection(op, state)), 0)
            if 0 < n < 3:
                return 100.0
            # visits to keep in reserve: those that complete the projection values met once or twice, and three for every value of a small
            # projection that has not been met at all (a large one need not meet all of its values: each variable's values are enough)
            reserve = owed[w] + (3 * (values[w] - filled[w] - started[w]) if values[w] <= 6 else 6)
            if n == 0:
                return 6.0 - 2.0 * len(op.proj) if left[w] - 3 >= owed[w] else -60.0
            return 10.0 if left[w] - 1 >= reserve else -50.0
        (var, val), = op.sets.items()
        if state[var] == val:
            return 8.0
        moved = {**state, var: val}         # a move towards the started projection values comes before a move away from them
        return -10.0 + sum(1.0 for q, pv in started_keys if projection(by[q], moved) == pv) - sum(0.5 for q, pv in started_keys if projection(by[q], state) == pv)

    def visit(name, counted=True):
        op = by[name]
        if op.kind == "setter":
            state.update(op.sets)
            return
        k = (name, projection(op, state))
        count[k] = count.get(k, 0) + 1
        if count[k] == 1:
            started[name] += 1
            owed[name] += 2
            started_keys.add(k)
        elif count[k] <= 3:
            owed[name] -= 1
            if count[k] == 3:
                started[name] -= 1
                filled[name] += 1
                started_keys.discard(k)
        left[name] -= counted

    at, seq = root, [root]
    visit(root, counted=False)              # the walk's first entry has no edge into it
    while unused[at]:
        cand = unused[at] if (at == root or len(unused[at]) == 1) else [w for w in unused[at] if w != root]
        nxt = max(cand, key=score)          # max keeps the first of equals: the seed's order
        unused[at].remove(nxt)
        visit(nxt)
        seq.append(nxt)
        at = nxt
    assert len(seq) == len(order) ** 2 + 1 and at == root
    _WALKS[key] = tuple(seq)
    return seq


def trajectory(ops, steps):
    """the logical state BEFORE every entry of the walk"""
    by = {o.name: o for o in ops}
    state, out = initial(ops), []
    for name in steps:
        out.append(dict(state))
        if by[name].kind == "setter":
            state.update(by[name].sets)
    return out


def projection(op, state):
    return tuple(state[v] for v in op.proj)


def visits(ops, steps):
    """(query, projection value) -> the predecessors it was visited after (None: the first entry of the walk)"""
    by = {o.name: o for o in ops}
    out = {}
    for i, (name, state) in enumerate(zip(steps, trajectory(ops, steps))):
        if by[name].kind == "query":
            out.setdefault((name, projection(by[name], state)), []).append(steps[i - 1] if i else None)
    return out


def coverage_problems(ops, steps, least=3):
    """What the coverage condition misses: a (query, projection value) visited fewer than `least` times or after fewer than `least` different
    predecessors; a query that never meets some value of a variable of its projection."""
    seen = visits(ops, steps)
    bad = [f"{q} in {pv}: {len(pr)} visits after {len(set(pr))} different predecessors" for (q, pv), pr in sorted(seen.items())
           if len(pr) < least or len(set(pr)) < least]
    for o in ops:
        if o.kind != "query":
            continue
        if not any(q == o.name for q, _ in seen):
            bad.append(f"{o.name} is never visited")
        for j, v in enumerate(o.proj):
            missing = domain(ops)[v] - {pv[j] for (q, pv) in seen if q == o.name}
            if missing:
                bad.append(f"{o.name} never runs with {v} in {sorted(missing)}")
    return bad


# ------------------------------------------------------------------------------------------------------------------ the run

Finding = namedtuple("Finding", "op predecessors state output index first now step")


def describe(f):
    return (f"{f.op} (step {f.step}) after {list(f.predecessors)} in state {f.state}: output {f.output!r} differs from the first result of this "
            f"(query, projection) at index {f.index}: first {f.first!r}, now {f.now!r}")


def first_difference(a, b, close=None):
    """results are dicts output -> array (or number); -> (output, index, first, now) of the first entry whose BITS differ, None if none does.
    close: (rtol, atol) for an operation that was demoted (see tests/test_gpu_handle_history.py: none is unless the fresh-pair test forces it)"""
    if sorted(a) != sorted(b):
        return ("<the set of outputs>", -1, sorted(a), sorted(b))
    for k in a:
        x, y = np.atleast_1d(np.asarray(a[k])), np.atleast_1d(np.asarray(b[k]))
        if x.shape != y.shape or x.dtype != y.dtype:
            return (k, -1, (x.shape, str(x.dtype)), (y.shape, str(y.dtype)))
        x, y = np.ascontiguousarray(x).ravel(), np.ascontiguousarray(y).ravel()
        if x.dtype.kind in "fiu" and x.dtype.itemsize == 8:
            differs = x.view(np.uint64) != y.view(np.uint64)
        else:
            differs = np.array([p != q for p, q in zip(x.tolist(), y.tolist())], dtype=bool)
        if close is not None and x.dtype.kind == "f":
            differs &= ~np.isclose(y, x, rtol=close[0], atol=close[1], equal_nan=True)
        bad = np.flatnonzero(differs)
        if bad.size:
            return (k, int(bad[0]), x[bad[0]].item(), y[bad[0]].item())
    return None


def seed_expected(make, ops, walks, expected, only=None, close=None):
    """For every (query, projection value) the walks meet and `expected` does not hold: the result of a backend made for it alone (make()), put
    STRAIGHT into that projection value from the default state.  A walk alone compares a handle with its own past: a value that is wrong
    in the same way on every visit -- a cache that a setter never invalidates, met only after long stays in one state -- passes it; the fresh
    result does not share the history.  only: one query's name."""
    by = {o.name: o for o in ops}
    setter = {item: o for o in ops if o.kind == "setter" for item in o.sets.items()}
    for q, pv in sorted({k for steps in walks for k in visits(ops, steps)}):
        if (only is not None and q != only) or (q, pv) in expected:
            continue
        backend, state = make(), initial(ops)
        try:
            for var, val in zip(by[q].proj, pv):
                if state[var] != val:
                    backend.setter(setter[(var, val)], dict(state))
                    state[var] = val
            expected[(q, pv)] = backend.query(by[q], dict(state))
        finally:
            if close is not None:
                close(backend)
    return expected


def run(backend, ops, steps, expected=None, demoted=None):
    """Drive backend.setter(op, state) / backend.query(op, state) -> result along the walk.  expected: (query, projection value) -> result, filled
    with every first occurrence it does not hold yet.  Returns the findings; an exception of the backend passes through."""
    by = {o.name: o for o in ops}
    expected = {} if expected is None else expected
    state, findings = initial(ops), []
    for i, name in enumerate(steps):
        op = by[name]
        if op.kind == "setter":
            backend.setter(op, dict(state))
            state.update(op.sets)
            continue
        res = backend.query(op, dict(state))
        key = (name, projection(op, state))
        if key not in expected:
            expected[key] = res
            continue
        d = first_difference(expected[key], res, (demoted or {}).get(name))
        if d is not None:
            findings.append(Finding(name, tuple(steps[max(0, i - 3):i]), dict(state), d[0], d[1], d[2], d[3], i))
    return findings
