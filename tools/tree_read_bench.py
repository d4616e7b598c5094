#!/usr/bin/env python3
"""What the tree read-out (az_search_read_tree / az_search_read_pv) costs, beside the only
alternative a caller had: a device-to-host copy of the whole arenas.

Subject: 256 games x 800 simulations from the startpos on a 10x128 f32 net (random-init, noise on, FEN cache
off), searched once.  Timed, as wall time around a block closed by a device synchronise, one warm-up and
three repeats each:
  read_tree of all games (the sizing call and the filling call, states included: BatchedSearch.read_tree_arrays),
  read_tree of one game, read_tree with max_depth = 0 (the roots alone), read_pv (cap 64),
  and a device-to-host copy of as many bytes as the same games' node, position, edge and child-header arenas
  hold (az_search_stats' node_cap / edge_cap: 16 + 80 B a node slot, 16 + 4 B an edge slot) from one device
  buffer into pageable host memory -- the arenas themselves are not exposed, the copy stands in for them.
The bytes each moves to the host are reported beside the times.  The numbers are not a gate.

    python tools/tree_read_bench.py [--games 256] [--sims 800] [--blocks 10] [--filters 128] [--repeats 3]
                                    [--out profiles/tree_read_bench.txt]
"""
import argparse
import ctypes
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "alphazero-chess_amd"))


def emit(lines, text):
    lines.append(text)
    print(text, flush=True)


def timed(A, fn, repeats):
    """one warm-up, then `repeats` wall times (ms) of fn() + a device synchronise -> (times, fn's last result)"""
    sync = lambda: A._lib.check(A._lib.lib.az_device_synchronize(ctypes.c_int(0)))
    out = fn()
    sync()
    ms = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = fn()
        sync()
        ms.append(1e3 * (time.perf_counter() - t0))
    return ms, out


def export_bytes(arrays):
    noff, eoff, nodes, edges, states = arrays
    return noff.nbytes + eoff.nbytes + nodes.nbytes + edges.nbytes + (0 if states is None else states.nbytes)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=256)
    ap.add_argument("--sims", type=int, default=800)
    ap.add_argument("--blocks", type=int, default=10)
    ap.add_argument("--filters", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tree_read_bench.txt"))
    args = ap.parse_args()
    import azchess as A
    from azchess.hiprt import Hip
    G = args.games
    lines = []
    net = A.AlphaZero(args.blocks, args.filters, weights=A.random_weights(args.blocks, args.filters, seed=42), dtype="f32")
    s = A.BatchedSearch(net, games=G, sims=args.sims, noise=True, seed=7, cache_capacity=0)
    s.set_roots([[] for _ in range(G)], apply_noise=True)
    t0 = time.perf_counter()
    s.run()
    emit(lines, "tree read-out: %d games x %d sims x %dx%d f32 (random-init, seed 42), searched once in %.2f s; "
         "persistent kernel %s; wall ms around a synchronised block, one warm-up + %d repeats"
         % (G, args.sims, args.blocks, args.filters, time.perf_counter() - t0, s.persistent, args.repeats))
    st = s.stats()
    emit(lines, " arenas: node_cap %d, edge_cap %d a game; live: at most %d nodes, %d edges a game"
         % (st["node_cap"], st["edge_cap"], st["max_nodes"], st["max_edges"]))

    def row(name, ms, nbytes, extra=""):
        emit(lines, " %-34s ms %s  (median %.3f)  %11d B to the host%s"
             % (name, " ".join("%.3f" % x for x in ms), sorted(ms)[len(ms) // 2], nbytes, extra))

    ms, arr = timed(A, lambda: s.read_tree_arrays(states=True), args.repeats)
    row("read_tree, all games, states", ms, export_bytes(arr), "  %d nodes, %d edges" % (len(arr[2]), len(arr[3])))
    full = export_bytes(arr)
    ms, arr = timed(A, lambda: s.read_tree_arrays(states=False), args.repeats)
    row("read_tree, all games, no states", ms, export_bytes(arr))
    ms, arr = timed(A, lambda: s.read_tree_arrays(games=[G // 2], states=True), args.repeats)
    row("read_tree, one game, states", ms, export_bytes(arr), "  %d nodes, %d edges" % (len(arr[2]), len(arr[3])))
    ms, arr = timed(A, lambda: s.read_tree_arrays(max_depth=0, states=True), args.repeats)
    row("read_tree, max_depth = 0, states", ms, export_bytes(arr), "  %d nodes, %d edges" % (len(arr[2]), len(arr[3])))
    ms, pv = timed(A, lambda: s.read_pv(64), args.repeats)
    row("read_pv, cap 64", ms, G * (64 * 4 + 12), "  mean length %.1f" % (sum(len(m) for m in pv[0]) / G))
    ms, _ = timed(A, s.read_roots, args.repeats)
    row("read_roots (for scale)", ms, G * (2 * 4096 * 4 + 4))

    # the alternative: the arenas as they are
    hip = Hip()
    per_game = st["node_cap"] * (16 + 80) + st["edge_cap"] * (16 + 4)
    for name, games in (("raw arena copy, all games", G), ("raw arena copy, one game", 1)):
        nbytes = per_game * games
        dev = hip.malloc(nbytes)
        host = np.empty(nbytes, np.uint8)
        ms, _ = timed(A, lambda: hip.download(dev, host), args.repeats)
        row(name, ms, nbytes)
        hip.free(dev)
    emit(lines, " the export of all games is %.1f %% of the arenas' bytes" % (100.0 * full / (per_game * G)))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
