#!/usr/bin/env python3
"""Owner-rank IBM markers, COUNTED from geometry on the CPU (no GPU, no library): for config 5's cylinder -- diameter 64 h along the periodic span,
one ring of 201 markers per z plane, as bench.py builds it for one block -- on the 1024 x 1024 x 512 grid over 2 x 2 x 2 ranks: markers owned,
ghost markers held and copies sent per rank, and the bytes on the wire per interp (3 components) and per spread against the all-reduce of 3 L
doubles that replicated markers need.  The rule is the one of include/fluca_hip.h: owner = the block of the cell floor(s + 1/2); a copy for
every other block that holds a cell of the support.

usage: python tools/ibm_owner_count.py [--centre X Y]        (default: the line where the four x-y blocks meet, the worst place)"""
import argparse
import json

import numpy as np


def count(n, ranks, periodic, h, X, S):
    L = X[0].size
    own_c, touch = [], []
    for a in range(3):
        m = ranks[a]
        q, r = divmod(n[a], m)
        lo = np.array([q * c + min(c, r) for c in range(m)])          # DMStag's split
        coord_of = lambda cell: np.searchsorted(lo, cell, side="right") - 1
        s = X[a] / h - 0.5
        c = np.floor(s + 0.5).astype(int)
        c = c % n[a] if periodic[a] else np.clip(c, 0, n[a] - 1)
        own_c.append(coord_of(c))
        i0 = (np.floor(s).astype(int) if S == 4 else np.floor(s + 0.5).astype(int)) - 1
        t = np.zeros((L, m), dtype=bool)
        for k in range(S):
            cell = i0 + k
            ok = np.ones(L, dtype=bool) if periodic[a] else (cell >= 0) & (cell < n[a])
            cell = cell % n[a]
            t[np.nonzero(ok)[0], coord_of(cell[ok])] = True
        touch.append(t)
    owner = (own_c[2] * ranks[1] + own_c[1]) * ranks[0] + own_c[0]
    T = np.einsum("lk,lj,li->lkji", touch[2], touch[1], touch[0]).reshape(L, -1)      # marker l touches rank (k, j, i)
    nr = ranks[0] * ranks[1] * ranks[2]
    owned = np.bincount(owner, minlength=nr)
    ghosts = T.sum(axis=0) - owned
    sent = np.bincount(owner, weights=T.sum(axis=1) - 1, minlength=nr).astype(int)
    return owned, ghosts, sent


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--centre", type=float, nargs=2, default=[0.5, 0.5])
    a = ap.parse_args()
    n, ranks, periodic, h = (1024, 1024, 512), (2, 2, 2), (False, False, True), 1.0 / 1024
    R = 32 * h
    nth = int(round(2 * np.pi * R / h))
    th = (np.arange(nth) + 0.5) * 2 * np.pi / nth
    z = (np.arange(n[2]) + 0.5) * h
    X = [np.tile(a.centre[0] + R * np.cos(th), n[2]), np.tile(a.centre[1] + R * np.sin(th), n[2]), np.repeat(z, nth)]
    L = X[0].size
    for kind, S in (("peskin4", 4), ("roma3", 3)):
        owned, ghosts, sent = count(n, ranks, periodic, h, X, S)
        copies = int(sent.sum())
        assert copies == int(ghosts.sum()) and int(owned.sum()) == L
        print(json.dumps(dict(counted_not_measured=True, delta=kind, centre=a.centre, markers=L, owned_per_rank=owned.tolist(), ghosts_per_rank=ghosts.tolist(),
                              copies_sent_per_rank=sent.tolist(), copies=copies, interp_bytes_all_ranks=24 * copies, spread_bytes_all_ranks=32 * copies,
                              interp_bytes_max_rank=int(24 * ghosts.max()), spread_bytes_max_rank=int(32 * sent.max()),
                              replicated_allreduce_bytes_per_rank=24 * L, wavefronts_per_rank_owned=int((owned + ghosts).max()), wavefronts_per_rank_replicated=L)))


if __name__ == "__main__":
    main()
