#!/usr/bin/env python3
"""What an MCTS player's ply costs in the match engine, and what leaf-parallel search does to its play.

Its legs, all on the engine's own stream (u = NULL), 10x128 f32 nets unless told otherwise:
  A  the two switches read at create -- AZ_ARENA_DEVICE_ROOTS (roots written by k_match_roots, or replayed on
     the host and uploaded) x AZ_ARENA_OVERLAP (a ply's searches side by side, or one after the other) -- on
     Tournaments of two and of three MCTS players on distinct nets, 64 games per match, 8 plies, 64
     simulations; once more with three players at 800 simulations.  All four forms play the same games.
  B  the same three players at leaves 1, 2, 4, 8 (the default switches): ms per ply, rows per forward.
  C  strength, a record and not a pass / fail: matches of 256 games played to their ends, ONE net on both
     sides (random-init: no trained checkpoint exists here) -- leaves 8 and 4 against leaves 1 at 64
     simulations, and two matches that show what the instrument resolves at all on such a net: 64 against 8
     simulations, and 64 simulations against the random player.  Win / draw / loss of player 1, its score
     (wins + draws / 2) / games and the 95 % Wilson interval of that score taken as a binomial rate.
  D  leg C's first match again at 800 simulations (minutes; not among the default legs).

One process: per case one warm-up of every form, then alternated repeats; wall time around blocks whose every
step ends in a stream synchronise (handles are created before the clock starts; their reset is inside it).

    python tools/arena_mcts_bench.py [--legs ABC] [--repeats 3] [--out profiles/arena_mcts_bench.txt]
    python tools/arena_mcts_bench.py --legs D --out profiles/arena_mcts_bench_800.txt
"""
import argparse
import contextlib
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "alphazero-chess_amd"))


@contextlib.contextmanager
def env(**kw):
    old = {k: os.environ.get(k) for k in kw}
    try:
        for k, v in kw.items():
            os.environ[k] = str(v)
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def run(tour, seed, max_plies):
    """(seconds, plies, forwards, rows) of one tournament from reset to max_plies or its end."""
    t0 = time.perf_counter()
    tour.reset(seed=seed)
    plies = 0
    while plies < max_plies:
        plies += 1
        if tour.step() == 0:
            break
    dt = time.perf_counter() - t0
    ninf, rows = tour.stats()
    return dt, plies, ninf, rows


def histories(tour):
    return [tour.history(m, g) for m in range(len(tour.matches)) for g in range(tour.games)]


def emit(lines, text):
    lines.append(text)
    print(text, flush=True)


def leg_a(V, nets, n_players, games, sims, plies, repeats, device, lines):
    players = [V.Player.mcts(n) for n in nets[:n_players]]
    forms = [(r, o) for o in (0, 1) for r in (0, 1)]           # (device roots, overlap)
    tours = {}
    for r, o in forms:
        with env(AZ_ARENA_DEVICE_ROOTS=r, AZ_ARENA_OVERLAP=o):
            tours[(r, o)] = V.Tournament(players, games=games, sims=sims, device=device)
    emit(lines, " A: %d MCTS players on distinct nets (%d matches), %d games per match, %d sims, %d plies"
         % (n_players, len(tours[(0, 0)].matches), games, sims, plies))
    for f in forms:
        run(tours[f], 1, 1 if sims > 200 else 2)               # warm-up
    ms = {f: [] for f in forms}
    same = True
    for rep in range(repeats):
        ref = None
        for f in forms:
            dt, n, ninf, rows = run(tours[f], 100 + rep, plies)
            h = histories(tours[f])
            ref = h if ref is None else ref
            ok = h == ref
            same = same and ok
            ms[f].append(dt * 1e3 / n)
            emit(lines, "  repeat %d roots %-6s overlap %-3s %9.1f ms, %9.3f ms per ply (%d plies, %.0f forwards, %.1f rows "
                 "per forward), move lists equal to host / off: %s"
                 % (rep, "device" if f[0] else "host", "on" if f[1] else "off", dt * 1e3, dt * 1e3 / n, n, ninf,
                    rows / max(ninf, 1.0), ok))
    # a switch is faster where it wins in every repeat of every pairing with the other switch's two values
    roots_faster = all(ms[(1, o)][k] < ms[(0, o)][k] for o in (0, 1) for k in range(repeats))
    overlap_faster = all(ms[(r, 1)][k] < ms[(r, 0)][k] for r in (0, 1) for k in range(repeats))
    emit(lines, "  device roots faster in every repeat: %s; overlap faster in every repeat: %s; move lists equal: %s"
         % (roots_faster, overlap_faster, same))
    mean = {f: sum(v) / len(v) for f, v in ms.items()}
    emit(lines, "  mean ms per ply: host/off %.3f, device/off %.3f, host/on %.3f, device/on %.3f"
         % (mean[(0, 0)], mean[(1, 0)], mean[(0, 1)], mean[(1, 1)]))
    return roots_faster, overlap_faster, same


def leg_b(V, nets, games, sims, plies, repeats, device, lines):
    emit(lines, " B: 3 MCTS players on distinct nets, %d games per match, %d sims, %d plies, by leaves" % (games, sims, plies))
    tours = {k: V.Tournament([V.Player.mcts(n, leaves=k) for n in nets[:3]], games=games, sims=sims, device=device)
             for k in (1, 2, 4, 8)}
    for k in tours:
        run(tours[k], 1, 2)
    for rep in range(repeats):
        for k, tour in tours.items():
            dt, n, ninf, rows = run(tour, 100 + rep, plies)
            emit(lines, "  repeat %d leaves %d %9.1f ms, %9.3f ms per ply (%d plies, %.0f forwards, %.1f rows per forward)"
                 % (rep, k, dt * 1e3, dt * 1e3 / n, n, ninf, rows / max(ninf, 1.0)))


def wilson(p, n, z=1.959964):
    d = 1.0 + z * z / n
    c = p + z * z / (2 * n)
    h = z * math.sqrt(p * (1.0 - p) / n + z * z / (4.0 * n * n))
    return (c - h) / d, (c + h) / d


def leg_c(V, L, net, games, device, lines, big):
    emit(lines, " %s: strength, %d games per match played to their ends, one random-init net on both sides"
         % ("D" if big else "C", games))
    M = V.Player.mcts
    cases = [("MCTS(64 sims, leaves 8) v MCTS(64 sims, leaves 1)", M(net, sims=64, leaves=8), M(net, sims=64)),
             ("MCTS(64 sims, leaves 4) v MCTS(64 sims, leaves 1)", M(net, sims=64, leaves=4), M(net, sims=64)),
             ("MCTS(64 sims) v MCTS(8 sims)", M(net, sims=64), M(net, sims=8)),
             ("MCTS(64 sims) v Random", M(net, sims=64), V.Player.random())]
    if big:
        cases = [("MCTS(%d sims, leaves 8) v MCTS(%d sims, leaves 1)" % (big, big), M(net, sims=big, leaves=8),
                  M(net, sims=big))]
    for name, p1, p2 in cases:
        arena = V.Arena(p1, p2, games=games, sims=64, seed=77, device=device)
        t0 = time.perf_counter()
        arena.reset(seed=77)
        plies = 0
        while plies < 420:
            plies += 1
            if arena.step() == 0:
                break
        dt = time.perf_counter() - t0
        res, npl = arena.results()
        w = d = l = open_ = 0
        for g, r in enumerate(res):
            r = int(r)
            if r == L.ONGOING:
                open_ += 1
            elif r == L.DRAW:
                d += 1
            elif (r == L.WHITE_WINS) == (g % 2 == 0):           # player 1 is White in the even games
                w += 1
            else:
                l += 1
        n = w + d + l
        score = (w + 0.5 * d) / max(n, 1)
        lo, hi = wilson(score, max(n, 1))
        emit(lines, "  %-52s +%d =%d -%d (unfinished %d): score %.3f, 95 %% interval %.3f..%.3f; %d plies, mean game %.1f "
             "plies, %.1f s" % (name, w, d, l, open_, score, lo, hi, plies, float(npl.mean()), dt))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="ABC")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--blocks", type=int, default=10)
    ap.add_argument("--filters", type=int, default=128)
    ap.add_argument("--games", type=int, default=64)
    ap.add_argument("--sims", type=int, default=64)
    ap.add_argument("--plies", type=int, default=8)
    ap.add_argument("--big-sims", type=int, default=800)
    ap.add_argument("--big-plies", type=int, default=3)
    ap.add_argument("--strength-games", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "arena_mcts_bench.txt"))
    a = ap.parse_args()
    import azchess as A
    from azchess import _lib as L
    from azchess import validation as V
    nets = [A.AlphaZero(a.blocks, a.filters, dtype="f32", device=a.device, seed=s) for s in (31, 32, 33)]
    lines = []
    emit(lines, "arena_mcts_bench %dx%d f32 (%s), the engine's own stream" % (a.blocks, a.filters, nets[0].tower_kernel))
    verdicts = []
    if "A" in a.legs:
        verdicts.append(leg_a(V, nets, 2, a.games, a.sims, a.plies, a.repeats, a.device, lines))
        verdicts.append(leg_a(V, nets, 3, a.games, a.sims, a.plies, a.repeats, a.device, lines))
        verdicts.append(leg_a(V, nets, 3, a.games, a.big_sims, a.big_plies, 1, a.device, lines))
        emit(lines, " A: device roots faster in every repeat of every case: %s; overlap faster in every repeat of every "
             "case: %s; move lists equal everywhere: %s"
             % (all(v[0] for v in verdicts), all(v[1] for v in verdicts), all(v[2] for v in verdicts)))
    if "B" in a.legs:
        leg_b(V, nets, a.games, a.sims, a.plies, a.repeats, a.device, lines)
    if "C" in a.legs:
        leg_c(V, L, nets[0], a.strength_games, a.device, lines, 0)
    if "D" in a.legs:
        leg_c(V, L, nets[0], a.strength_games, a.device, lines, a.big_sims)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    assert all(v[2] for v in verdicts), "the forms of leg A played different moves"
    return 0


if __name__ == "__main__":
    sys.exit(main())
