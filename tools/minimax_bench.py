#!/usr/bin/env python3
"""Throughput of the MiniMax bot's scoring (az_minimax_scores): the GPU kernels against the host
path (at most 16 threads) on one batch of positions from seeded random playouts, built with the
engine's own host rules.  One warm-up call each, then alternated repeats; wall time around the
call (it returns after its stream has been synchronised); nodes/s from the returned call counts.

    python tools/minimax_bench.py [--positions 128] [--depth 4] [--repeats 3] [--out profiles/minimax_bench.txt]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "alphazero-chess_amd"))

import azchess as A  # noqa: E402
from azchess import chess as CH  # noqa: E402


def playout_positions(count, seed, games=16, max_plies=100):
    """`count` positions with a legal move, at evenly spaced points of uniform random playouts"""
    rng = np.random.default_rng(seed)
    seen = []
    for _ in range(games):
        state = A.GameState()
        for _ in range(max_plies):
            pos = state.position
            legal = pos.legal_indices()
            seen.append(pos)
            if int(A.play_move(state, int(legal[rng.integers(len(legal))]))) != 0:
                break
    idx = np.linspace(0, len(seen) - 1, count).astype(int)
    return [seen[i] for i in idx]


def timed(positions, depth, device):
    t0 = time.perf_counter()
    entries, nodes = CH.minimax_scores(positions, depth, device)
    return time.perf_counter() - t0, entries, nodes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--positions", type=int, default=128)
    ap.add_argument("--depth", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--seed", type=int, default=11)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "minimax_bench.txt"))
    a = ap.parse_args()
    positions = CH.positions_to_array(playout_positions(a.positions, a.seed))
    lines = []
    _, ge, gn = timed(positions, a.depth, a.device)               # warm-up, and the parity check
    _, he, hn = timed(positions, a.depth, CH.DEVICE_HOST)
    same = np.array_equal(gn, hn) and all(np.array_equal(x, y) for g, h in zip(ge, he) for x, y in zip(g, h))
    total = int(hn.sum())
    lines.append("minimax_bench: %d positions, depth %d, %d negamax calls, frontier %s nodes, GPU == host: %s"
                 % (a.positions, a.depth, total, os.environ.get("AZ_MINIMAX_FRONTIER", "default"), same))
    best = {}
    for r in range(a.repeats):
        for name, dev in (("gpu", a.device), ("host16", CH.DEVICE_HOST)):
            dt, _, nodes = timed(positions, a.depth, dev)
            best[name] = min(best.get(name, dt), dt)
            lines.append("repeat %d %-6s %9.2f ms  %8.1f M nodes/s" % (r, name, dt * 1e3, nodes.sum() / dt / 1e6))
    lines.append("best gpu %.2f ms (%.1f M nodes/s), best host16 %.2f ms (%.1f M nodes/s), ratio %.2f"
                 % (best["gpu"] * 1e3, total / best["gpu"] / 1e6, best["host16"] * 1e3, total / best["host16"] / 1e6,
                    best["host16"] / best["gpu"]))
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
