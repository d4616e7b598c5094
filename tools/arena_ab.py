#!/usr/bin/env python3
"""The games of a fixed list of arena and tournament configurations, for comparing two builds of libaz
(AZ_LIB selects the build): every pairing of {base, MCTS with a net, MCTS synthetic, MiniMax(1), random},
base against another base net, a player against itself, an external seat, given start positions with
mixed sides to move, and one tournament of four players.  2x32 f32 nets, 4-6 games, 8 simulations, 24 plies,
num_stochastic_moves 3; every configuration once on the engine's own stream (u = NULL) and once with
given uniforms.

Prints, per configuration, the results, plies, live mask, statistics and move lists, and last a SHA-256
digest of all of it.  Two builds play the same games exactly when their outputs are byte-identical.  The
move lists depend on the tower kernels' last bits, so they are compared between builds of one tree, never
kept as a fixture.

    python tools/arena_ab.py [--out FILE]
"""
import argparse
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "alphazero-chess_amd"))

SIMS, PLIES, NSM = 8, 24, 3
START_FENS = [                                               # White, Black, Black, White, White to move
    "rnbqkbnr/pppppppp/8/8/8/8/PPPPPPPP/RNBQKBNR w KQkq - 0 1",
    "rnbqkbnr/pppppppp/8/8/4P3/8/PPPP1PPP/RNBQKBNR b KQkq - 0 1",
    "rnbqkbnr/pppppppp/8/8/3P4/8/PPP1PPPP/RNBQKBNR b KQkq - 0 1",
    "rnbqkb1r/pppppppp/5n2/8/8/5N2/PPPPPPPP/RNBQKB1R w KQkq - 2 2",
    "4k3/8/8/8/8/8/8/R3K3 w - - 90 80",
]


def uniforms(seed, ply, n):
    return np.random.default_rng([seed, ply]).random(n, dtype=np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import azchess as A
    from azchess import validation as V
    nets = [A.AlphaZero(2, 32, dtype="f32", device=a.device, seed=s) for s in (4, 5)]
    kinds = {
        "base": lambda: V.Player.base(nets[0]),
        "mcts_net": lambda: V.Player.mcts(nets[1]),
        "mcts_syn": lambda: V.Player.mcts(None),
        "minimax1": lambda: V.Player.minimax(1),
        "random": lambda: V.Player.random(),
    }
    names = list(kinds)
    lines = []

    def report(name, stream, handle, hist):
        res, plies = handle.results()
        ninf, rows = handle.stats()
        lines.append("%s [%s] results %s plies %s live %s num_inferences %r rows %r"
                     % (name, stream, res.reshape(-1).tolist(), plies.reshape(-1).tolist(),
                        handle.live().reshape(-1).astype(int).tolist(), ninf, rows))
        for k, h in enumerate(hist):
            lines.append("  %d: %s" % (k, " ".join(map(str, h))))

    def arena(name, p1, p2, games, seed, start=None, external=False):
        h = V.Arena(p1, p2, games=games, sims=SIMS, num_stochastic_moves=NSM, seed=seed, device=a.device)
        for stream in ("own", "given"):
            h.reset(start=start, seed=seed)
            pos = list(start) if start else [A.Position.startpos() for _ in range(games)]
            for ply in range(PLIES):
                actions = None
                if external:                                 # an external seat plays a fixed legal move
                    live = h.live()
                    actions = np.full(games, -1, np.int32)
                    for g in np.flatnonzero(live):
                        legal = pos[g].legal_indices()
                        actions[g] = int(legal[(3 * g + ply) % len(legal)])
                n = h.step(u=uniforms(seed, ply, games) if stream == "given" else None, actions=actions)
                if external:
                    for g in np.flatnonzero(live):
                        pos[g] = pos[g].play(h.history(int(g))[-1])
                if n == 0:
                    break
            report(name, stream, h, [h.history(g) for g in range(games)])

    seed = 100
    for i, k1 in enumerate(names):                           # every pairing of the five kinds
        for k2 in names[i + 1:]:
            seed += 1
            arena("%s vs %s" % (k1, k2), kinds[k1](), kinds[k2](), 4 + seed % 3, seed)
    arena("base vs base (another net)", V.Player.base(nets[0]), V.Player.base(nets[1]), 6, 121)
    for k in ("base", "mcts_net", "mcts_syn"):                # one player on both sides
        seed += 1
        p = kinds[k]()
        arena("%s vs itself" % k, p, p, 5, seed)
    arena("mcts_net vs external", kinds["mcts_net"](), V.Player.external(), 5, 131, external=True)
    arena("external vs base", V.Player.external(), kinds["base"](), 4, 132, external=True)
    start = [A.Position.from_fen(f) for f in START_FENS]
    arena("base vs mcts_net from start positions", kinds["base"](), kinds["mcts_net"](), 5, 133, start=start)
    arena("mcts_syn vs minimax1 from start positions", kinds["mcts_syn"](), kinds["minimax1"](), 5, 134, start=start)

    players = [kinds[k]() for k in ("base", "mcts_net", "minimax1", "random")]
    tour = V.Tournament(players, games=4, sims=SIMS, num_stochastic_moves=NSM, seed=141, device=a.device)
    M = len(tour.matches)
    for stream in ("own", "given"):
        tour.reset(seed=141)
        for ply in range(PLIES):
            if tour.step(uniforms(141, ply, M * 4) if stream == "given" else None) == 0:
                break
        report("tournament base, mcts_net, minimax1, random", stream, tour,
               [tour.history(m, g) for m in range(M) for g in range(4)])

    text = "\n".join(lines) + "\n"
    text += "configurations %d, sha256 %s\n" % (sum(1 for s in lines if not s.startswith("  ")),
                                               hashlib.sha256(text.encode()).hexdigest())
    sys.stdout.write(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
