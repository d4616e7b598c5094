#!/usr/bin/env python3
"""What a round robin costs (ratings.rs:10-24): the pairings played one after the other, each on its own
Arena (what compute_elo_rankings(engine=True) does), against all of them in lockstep on one Tournament
(az_tournament_*: one forward or one search per player and ply over all of its matches).

Two legs, both on the engine's own stream (u = NULL, the same seed on both paths, so the games are the same):
  base  four base-model 10x128 f32 players, 256 games per match, played to the end (max 400 plies)
  mcts  three MCTS 10x128 f32 players, 64 games per match, 64 simulations, a fixed small number of plies

One process: one warm-up of each path, then alternated repeats; wall time around blocks whose every step
ends in a stream synchronise (the handles are created before the clock starts; their reset is inside it).
Per repeat and path: ms per tournament ply (the path's wall time over the plies of the longest match), the
average batch (rows / forwards), and whether all move lists are equal.

    python tools/tournament_bench.py [--repeats 3] [--out profiles/tournament_bench.txt]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "alphazero-chess_amd"))


def leg(name, players, games, sims, max_plies, repeats, device, lines):
    from azchess import validation as V
    tour = V.Tournament(players, games=games, sims=sims, device=device)
    arenas = [V.Arena(players[i], players[j], games=games, sims=sims, device=device) for i, j in tour.matches]

    def pairwise(seed, max_plies):
        t0 = time.perf_counter()
        plies = 0
        for arena in arenas:                                   # one match after the other
            arena.reset(seed=seed)
            n = 0
            while n < max_plies:
                n += 1
                if arena.step() == 0:
                    break
            plies = max(plies, n)
        dt = time.perf_counter() - t0
        ninf = sum(a.stats()[0] for a in arenas)
        rows = sum(a.stats()[1] for a in arenas)
        return dt, plies, rows / max(ninf, 1.0)

    def lockstep(seed, max_plies):
        t0 = time.perf_counter()
        tour.reset(seed=seed)
        plies = 0
        while plies < max_plies:
            plies += 1
            if tour.step() == 0:
                break
        dt = time.perf_counter() - t0
        ninf, rows = tour.stats()
        return dt, plies, rows / max(ninf, 1.0)

    pairwise(1, 4)                                             # warm-up: both paths, a few plies
    lockstep(1, 4)
    same, faster = True, True
    for r in range(repeats):
        tp, pp, bp = pairwise(100 + r, max_plies)
        tt, pt, bt = lockstep(100 + r, max_plies)
        ok = pp == pt and all(arenas[m].history(g) == tour.history(m, g)
                              for m in range(len(arenas)) for g in range(games))
        same, faster = same and ok, faster and tt < tp
        lines.append("  %s repeat %d pairwise   %9.1f ms, %8.3f ms per tournament ply (%d plies, avg batch %7.1f)"
                     % (name, r, tp * 1e3, tp * 1e3 / pp, pp, bp))
        lines.append("  %s repeat %d tournament %9.1f ms, %8.3f ms per tournament ply (%d plies, avg batch %7.1f), "
                     "pairwise / tournament %.2f, all move lists equal: %s"
                     % (name, r, tt * 1e3, tt * 1e3 / pt, pt, bt, tp / tt, ok))
    lines.append("  %s: tournament faster in every repeat: %s; move lists equal in every repeat: %s" % (name, faster, same))
    return same


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--blocks", type=int, default=10)
    ap.add_argument("--filters", type=int, default=128)
    ap.add_argument("--base-games", type=int, default=256)
    ap.add_argument("--base-max-plies", type=int, default=400)
    ap.add_argument("--mcts-games", type=int, default=64)
    ap.add_argument("--mcts-sims", type=int, default=64)
    ap.add_argument("--mcts-plies", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tournament_bench.txt"))
    a = ap.parse_args()
    import azchess as A
    from azchess import validation as V
    nets = [A.AlphaZero(a.blocks, a.filters, dtype="f32", device=a.device, seed=s) for s in (31, 32, 33, 34)]
    lines = ["tournament_bench %dx%d f32 (%s)" % (a.blocks, a.filters, nets[0].tower_kernel),
             " base leg: 4 base-model players (6 matches), %d games per match, max_plies %d, the engine's own stream"
             % (a.base_games, a.base_max_plies)]
    same = leg("base", [V.Player.base(n) for n in nets], a.base_games, 1, a.base_max_plies, a.repeats, a.device, lines)
    lines.append(" mcts leg: 3 MCTS players (3 matches), %d games per match, %d sims, %d plies, the engine's own stream"
                 % (a.mcts_games, a.mcts_sims, a.mcts_plies))
    same = leg("mcts", [V.Player.mcts(n) for n in nets[:3]], a.mcts_games, a.mcts_sims, a.mcts_plies, a.repeats,
               a.device, lines) and same
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    assert same, "the tournament and the pairwise arenas played different moves"
    return 0


if __name__ == "__main__":
    sys.exit(main())
