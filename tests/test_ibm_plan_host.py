"""The message plan of the owner-rank markers (fluca_amd/csrc/fl_ibm_plan.h) on the host, for every rank of four rank grids: RCCL matches the
messages between two ranks by their ORDER alone, and the transports the GPU tests run on carry tags -- so a list that broke the rule "sends in
ascending offset code, receives in descending" would pass every one of them and hang on the first real several-GPU run.  tests/plugins/ibm_plan_check.cpp
(plain g++, no HIP call) prints what the header plans; the judgement is here."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FACES = {4, 10, 12, 14, 16, 22}
GRIDS = {"2x1x1 periodic x": ((2, 1, 1), (1, 0, 0)), "1x1x2 periodic z": ((1, 1, 2), (0, 0, 1)), "2x2x2 periodic z": ((2, 2, 2), (0, 0, 1)),
         "3x2x2 no periodic axis": ((3, 2, 2), (0, 0, 0))}


def send_count(rank, code):
    """ibm_plan_check.cpp's: the records a rank sends under an offset; zero for some."""
    return (7 * rank + 3 * code + rank * code) % 4


@pytest.fixture(scope="module")
def check():
    """tests/plugins/ibm_plan_check.cpp built with g++ against the header and libflucahip.so (fl_decomp_default, fl_decomp_neighbor_offset)."""
    from fluca_amd import build
    build.build()
    out = os.path.join(ROOT, "tests", "plugins", "ibm_plan_check")
    src = os.path.join(ROOT, "tests", "plugins", "ibm_plan_check.cpp")
    csrc = os.path.join(ROOT, "fluca_amd", "csrc")
    libdir = os.path.join(ROOT, "fluca_amd", "lib")
    deps = [src, os.path.join(csrc, "fl_ibm_plan.h"), os.path.join(csrc, "fl_msg.h"), os.path.join(libdir, "libflucahip.so")]
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", out, src, "-L" + libdir, "-lflucahip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    return out


@pytest.fixture(scope="module", params=sorted(GRIDS))
def plan(request, check):
    ranks, periodic = GRIDS[request.param]
    text = subprocess.check_output([check] + [str(a) for a in ranks + periodic], text=True)
    coord, peer, msgs = {}, {}, {}
    for line in text.splitlines():
        w = line.split()
        if w[0] == "C":
            coord[int(w[1])] = tuple(int(a) for a in w[2:5])
        elif w[0] == "P":
            peer[(int(w[1]), int(w[2]))] = int(w[3])
        else:
            keys = ("kind", "code", "peer", "count", "offset", "sendtag", "recvtag")
            msgs.setdefault((w[1], int(w[2])), []).append(dict(zip(keys, [w[3]] + [int(a) for a in w[4:]])))
    nranks = ranks[0] * ranks[1] * ranks[2]
    assert sorted(coord) == list(range(nranks)) and len(set(coord.values())) == nranks
    return dict(name=request.param, ranks=ranks, periodic=periodic, nranks=nranks, coord=coord, peer=peer, msgs=msgs)


def _expected_peer(plan, rank, code):
    """The rank behind an offset from the ranks' coordinates alone: none across a wall, none along an axis that one rank holds alone."""
    o = (code % 3 - 1, (code // 3) % 3 - 1, code // 9 - 1)
    if code == 13:
        return -1
    c = list(plan["coord"][rank])
    for d in range(3):
        if o[d] == 0:
            continue
        if plan["ranks"][d] == 1:
            return -1
        c[d] += o[d]
        if not 0 <= c[d] < plan["ranks"][d]:
            if not plan["periodic"][d]:
                return -1
            c[d] %= plan["ranks"][d]
    return {v: k for k, v in plan["coord"].items()}[tuple(c)]


def test_peers(plan):
    for r in range(plan["nranks"]):
        for code in range(27):
            assert plan["peer"][(r, code)] == _expected_peer(plan, r, code), (plan["name"], r, code)
    if plan["name"] == "2x1x1 periodic x":   # both x offsets lead to the one other rank
        assert plan["peer"][(0, 12)] == plan["peer"][(0, 14)] == 1 and plan["peer"][(1, 12)] == plan["peer"][(1, 14)] == 0
    if plan["name"] == "1x1x2 periodic z":
        assert plan["peer"][(0, 4)] == plan["peer"][(0, 22)] == 1


@pytest.mark.parametrize("variant", ["records", "keep", "faces"])
def test_lists_of_every_rank(plan, variant):
    """Per rank: only offsets with a rank behind them, the tags (code, 26 - code), sends ascending before receives descending, the counts and places
    asked for, an empty message exactly when it is to be kept."""
    # the counts do have zeros: they are what "records" leaves out and "keep" keeps
    assert any(plan["peer"][(r, c)] >= 0 and send_count(r, c) == 0 for r in range(plan["nranks"]) for c in range(27))
    for r in range(plan["nranks"]):
        lst = plan["msgs"].get((variant, r), [])
        live = [c for c in range(27) if plan["peer"][(r, c)] >= 0 and (variant != "faces" or c in FACES)]
        for m in lst:
            assert m["code"] in live and m["peer"] == plan["peer"][(r, m["code"])], (plan["name"], r, m)
            assert (m["sendtag"], m["recvtag"]) == (m["code"], 26 - m["code"])
        sends, recvs = [m for m in lst if m["kind"] == "S"], [m for m in lst if m["kind"] == "R"]
        assert lst == sends + recvs
        if variant == "faces":
            assert {m["code"] for m in lst} <= FACES
            assert [m["code"] for m in sends] == live and [m["code"] for m in recvs] == live[::-1]
            assert all(m["count"] == 6 and m["offset"] == 0 for m in sends)
            assert all(m["count"] == 6 and m["offset"] == 6 * (1 + m["code"]) for m in recvs)
            continue
        scnt = {c: send_count(r, c) for c in live}
        rcnt = {c: send_count(plan["peer"][(r, c)], 26 - c) for c in live}
        keep = variant == "keep"
        assert [m["code"] for m in sends] == [c for c in live if keep or scnt[c] > 0]
        assert [m["code"] for m in recvs] == [c for c in live[::-1] if keep or rcnt[c] > 0]
        assert all(m["count"] == 3 * scnt[m["code"]] for m in sends) and all(m["count"] == 3 * rcnt[m["code"]] for m in recvs)
        # the records of an offset lie next to each other, the offsets in ascending code
        for side, cnt in ((sends, scnt), (recvs, rcnt)):
            for m in side:
                assert m["offset"] == 3 * sum(cnt[c] for c in live if c < m["code"])


@pytest.mark.parametrize("variant", ["records", "keep", "faces"])
def test_order_pairs_the_messages_of_every_two_ranks(plan, variant):
    """What a transport that matches by order alone does: the k-th send of a to b meets the k-th receive that b posts for a."""
    pairs = 0
    for a in range(plan["nranks"]):
        for b in range(plan["nranks"]):
            sends = [m for m in plan["msgs"].get((variant, a), []) if m["kind"] == "S" and m["peer"] == b]
            recvs = [m for m in plan["msgs"].get((variant, b), []) if m["kind"] == "R" and m["peer"] == a]
            assert len(sends) == len(recvs), (plan["name"], variant, a, b)
            for s, r in zip(sends, recvs):
                assert s["count"] == r["count"], (plan["name"], variant, a, b, s, r)
                assert s["sendtag"] == r["recvtag"] and r["code"] == 26 - s["code"], (plan["name"], variant, a, b, s, r)
            pairs += len(sends)
            if a == b:
                assert not sends       # none of the four grids sends to itself
    assert pairs > 0
    if plan["name"] == "2x1x1 periodic x" and variant != "records":
        assert len([m for m in plan["msgs"][(variant, 0)] if m["kind"] == "S" and m["peer"] == 1]) == 2    # two offsets, one peer: the case the rule is for
