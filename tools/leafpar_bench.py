#!/usr/bin/env python3
"""Leaf-parallel search (make_cfg(leaves=K): K leaves per game per simulation step), measured against one
leaf per step in the same process.  Legs (FEN cache off everywhere):

  tree-20x256, tree-10x128   BatchedSearch(net, games=1, sims=800) from the start position: ms per move
  carried                    256 slots x 64 simulations, 10x128 f32, continuous self-play, 20 moves
  c2                         256 games x 800 simulations, 6x64 f32, continuous self-play, 3 moves
  full                       2048 games x 800 simulations, 20x256 f32, 2 moves, K in {1, 2} only

Per leg: one handle per K, one warm-up each, then `--repeats` rounds that take the Ks in turn.  Wall time
around a block that ends in a stream synchronise (run() reads the roots back; a self-play step ends in a
synchronised drain).  Per leg and K also: which step kernels ran (the persistent per-game kernel, or the
step kernel and the batched tower), network rows per simulation step, the share of simulations whose leaf
was shared, and the total-variation distance between the improved policies at K and at K = 1 on the same
noised start-position roots (one search of the leg's shape per K, untimed) -- the only search-quality figure
here.  Playing strength at K > 1 is not measured.

    python tools/leafpar_bench.py [--repeats 3] [--legs tree-20x256,carried,...] [--out profiles/leafpar_bench.txt]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "alphazero-chess_amd"))

#        name           blocks filters games sims  moves  Ks
LEGS = [("tree-20x256", 20, 256, 1, 800, 1, (1, 2, 4, 8)),
        ("tree-10x128", 10, 128, 1, 800, 1, (1, 2, 4, 8)),
        ("carried", 10, 128, 256, 64, 20, (1, 2, 4, 8)),
        ("c2", 6, 64, 256, 800, 3, (1, 2, 4, 8)),
        ("full", 20, 256, 2048, 800, 2, (1, 2))]


def counters(s):
    st = s.stats()
    return np.array([st["sims"], st["evals"], s.shared_leaves], np.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--legs", default=",".join(l[0] for l in LEGS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "leafpar_bench.txt"))
    a = ap.parse_args()
    import azchess as A
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    nets = {}
    for name, blocks, filters, games, sims, moves, Ks in LEGS:
        if name not in a.legs.split(","):
            continue
        if (blocks, filters) not in nets:
            nets[(blocks, filters)] = A.AlphaZero(blocks, filters, weights=A.random_weights(blocks, filters, seed=42),
                                                  dtype="f32", device=a.device)
        net = nets[(blocks, filters)]
        tree = games == 1
        say("%s: %dx%d f32 (%s), %d game%s x %d simulations, %s, %d repeats"
            % (name, blocks, filters, net.tower_kernel, games, "s" * (games > 1), sims,
               "search from the start position" if tree else "continuous self-play, %d moves a repeat" % moves, a.repeats))
        cfg = dict(games=games, sims=sims, device=a.device, seed=a.seed, cache_capacity=0)
        # the improved policies on the same roots, per K (untimed); for the one-tree legs also the timed handle
        imp, handles, kernel = {}, {}, {}
        for K in Ks:
            s = A.BatchedSearch(net, leaves=K, **cfg)
            s.set_roots([[]] * games, apply_noise=True)
            imp[K] = s.run()[0]
            kernel[K] = "persistent per-game kernel" if s.persistent else "step kernel + batched tower"
            if tree:
                handles[K] = s
            else:
                del s
                handles[K] = A.SelfPlay(net, continuous=True, leaves=K, **cfg)
                handles[K].reset()
                handles[K].step()                                   # warm-up
        walls = {K: [] for K in Ks}
        total = {K: np.zeros(3, np.int64) for K in Ks}
        for _ in range(a.repeats):
            for K in Ks:
                h = handles[K]
                srch = h if tree else h.search
                if tree:
                    h.set_roots([[]], apply_noise=True)
                c0 = counters(srch)
                t0 = time.perf_counter()
                if tree:
                    h.run()
                else:
                    for _ in range(moves):
                        h.step()
                        h.drain_raw()
                walls[K].append(time.perf_counter() - t0)
                total[K] += counters(srch) - c0
        for K in Ks:
            sims_done, evals, shared = (int(x) for x in total[K])
            steps = a.repeats * moves * -(-sims // K)
            tv = 0.5 * np.abs(imp[K].astype(np.float64) - imp[1].astype(np.float64)).sum(1)
            unit = [1e3 * w / moves for w in walls[K]] if tree else [games * sims * moves / w for w in walls[K]]
            say("  K = %d (%s): %s %s   rows per simulation step %.1f   shared leaves %.1f %%   TV to K = 1: mean %.3f max %.3f"
                % (K, kernel[K], "ms per move" if tree else "sims/s",
                   " ".join(("%.1f" if tree else "%.0f") % u for u in unit), evals / steps, 100.0 * shared / max(sims_done, 1),
                   tv.mean(), tv.max()))
        for K in Ks[1:]:
            wins = sum(x < y for x, y in zip(walls[K], walls[1]))
            say("  K = %d is faster than K = 1 in %d of %d repeats (x%.2f by the mean wall time)"
                % (K, wins, a.repeats, np.mean(walls[1]) / np.mean(walls[K])))
        handles.clear()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
