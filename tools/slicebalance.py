#!/usr/bin/env python3
"""How evenly an item's child slices load the waves of its workgroup (CPU only).

    python tools/slicebalance.py [--nodes 1024] [--events 1000000] [--kbar 8] [--waves 8] [--whole-nodes]

The data are bench.py's (synthetic.s_metric_data, seeded).  Items are cut as the library cuts them (cont_data.hip:
nhp_cont_partition without time parts; --whole-nodes: one item per node whatever its size), an item's children are sorted
longest window first and slice j holds children 64·j .. 64·j + 63, so its rows are its first child's window.  A wave's load is
the sum of the rows of its slices, and the workgroup lasts as long as its longest wave.  Three ways of dealing:

    forward   wave w takes slices w, w + NW, w + 2·NW, ...: wave 0 gets the longest slice of every round
    snake     round r forwards when r is even, backwards when odd (csrc/nhp_internal.h: nhp_slice_of; what the kernels do)
    greedy    longest slice first to the least loaded wave (would need a per-item table in the dataset: not built)

Printed: mean rows per wave, and per dealing the mean over items of the longest wave's rows with the worst item in brackets."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def slice_of(r, w, nw):
    """nhp_slice_of (tests/test_slices_walk_host.py holds the library's function to the same properties)"""
    return r * nw + (nw - 1 - w if r & 1 else w)


def item_slices(times, nodes, N, dt_max=1.0, whole_nodes=False):
    """Rows of every slice, item by item: a list of descending int arrays (an item without children gives an empty one)."""
    M = len(times)
    idx = np.arange(M)
    first = np.minimum(np.searchsorted(times, times - dt_max, side="right"), idx)      # parents: t_j > t_i - Δtmax, j < i
    wlen = idx - first
    chunk = int(1.3 * M / N) + 1 if N >= 1024 else (M + 1023) // 1024
    chunk = max(32, min(4096, chunk))
    order = np.argsort(nodes, kind="stable")
    bounds = np.searchsorted(nodes[order], np.arange(1, N + 2))
    out = []
    for c in range(N):
        kids = wlen[order[bounds[c]:bounds[c + 1]]]                                    # time order
        n = len(kids)
        parts = 1 if whole_nodes else max(1, -(-n // chunk))
        for q in range(parts):
            part = np.sort(kids[n * q // parts:n * (q + 1) // parts])[::-1]
            out.append(part[::64].astype(np.int64))
    return out, int(wlen.sum())


def longest_wave(rows, nw):
    """(forward, snake, greedy) rows of the longest wave for one item's slices."""
    ns = len(rows)
    fwd = max((int(rows[w::nw].sum()) for w in range(nw)), default=0)
    snake = 0
    for w in range(nw):
        load, r = 0, 0
        while slice_of(r, w, nw) < ns:
            load += int(rows[slice_of(r, w, nw)])
            r += 1
        snake = max(snake, load)
    loads = [0] * nw
    for v in rows:
        loads[loads.index(min(loads))] += int(v)
    return fwd, snake, max(loads)


def table(N, M, kbar, nw, whole_nodes=False):
    from __graft_entry__ import load_package
    nhp = load_package()
    times, nodes, T = nhp.synthetic.s_metric_data(N, M, kbar=kbar)
    items, pairs = item_slices(times, nodes, N, whole_nodes=whole_nodes)
    res = np.array([longest_wave(rows, nw) for rows in items], dtype=np.float64)
    total = np.array([rows.sum() for rows in items], dtype=np.float64)
    return {"items": len(items), "slices": int(sum(len(r) for r in items)), "pairs": pairs,
            "records_per_pair": 64.0 * total.sum() / max(pairs, 1), "slices_per_item": float(np.mean([len(r) for r in items])),
            "mean_rows_per_wave": float((total / nw).mean()),
            "forward": (float(res[:, 0].mean()), int(res[:, 0].max())), "snake": (float(res[:, 1].mean()), int(res[:, 1].max())),
            "greedy": (float(res[:, 2].mean()), int(res[:, 2].max()))}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--nodes", type=int, default=1024)
    ap.add_argument("--events", type=int, default=1_000_000)
    ap.add_argument("--kbar", type=float, default=8.0)
    ap.add_argument("--waves", type=int, default=8, help="waves per workgroup (BLOCK / 64)")
    ap.add_argument("--whole-nodes", action="store_true", help="one item per node, whatever the library's chunk")
    a = ap.parse_args()
    t = table(a.nodes, a.events, a.kbar, a.waves, a.whole_nodes)
    print(f"N {a.nodes}, M {a.events}, mean window {a.kbar:g}, {a.waves} waves: {t['items']} items, {t['slices_per_item']:.2f} slices per item, "
          f"{t['records_per_pair']:.3f} records per pair")
    print(f"mean rows per wave {t['mean_rows_per_wave']:.2f}")
    for k in ("forward", "snake", "greedy"):
        print(f"longest wave, {k:8s} {t[k][0]:7.2f} ({t[k][1]})")


if __name__ == "__main__":
    main()
