#!/usr/bin/env python3
"""What an evaluation match costs (validation.rs:155-282, EVALUATION_GAMES = 256 every iteration): the host
loop of validation.evaluate (per ply and game: to_tensor, the policy copied to the host, legal_indices,
a numpy mask and choice, play_move through ctypes) against the engine arena (evaluate(engine=True):
az_arena_step, games in HBM, only the uniforms go up and the results come down).  Base model 10x128
against base model 10x128 with different seeds, 256 games, max_plies 400, f32.

One process: one short warm-up of each path, then alternated repeats; wall time per match and per ply,
and a check that the two paths played the same moves in every game.  Both of those draw every (game, ply)
uniform from its own numpy generator (validation.choice_uniform), which is what keeps them equal; a third
line per repeat plays a match on the same Arena with the engine's own stream (u = NULL: other moves, so no
comparison) to show the arena without that host work.

    python tools/arena_bench.py [--repeats 3] [--out profiles/arena_bench.txt]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "alphazero-chess_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--games", type=int, default=256)
    ap.add_argument("--max-plies", type=int, default=400)
    ap.add_argument("--blocks", type=int, default=10)
    ap.add_argument("--filters", type=int, default=128)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "arena_bench.txt"))
    a = ap.parse_args()
    import azchess as A
    from azchess import validation as V
    nets = [A.AlphaZero(a.blocks, a.filters, dtype="f32", device=a.device, seed=s) for s in (31, 32)]
    p1, p2 = V.Player.base(nets[0]), V.Player.base(nets[1])

    def match(engine, max_plies, seed):
        t0 = time.perf_counter()
        res, hist, result = V.evaluate(p1, p2, games=a.games, seed=seed, device=a.device, max_plies=max_plies,
                                       record=True, engine=engine)
        return time.perf_counter() - t0, res, hist, result

    arena = V.Arena(p1, p2, games=a.games, device=a.device)

    def own_stream(seed):
        t0 = time.perf_counter()
        arena.reset(seed=seed)
        plies = 0
        while plies < a.max_plies:
            plies += 1
            if arena.step() == 0:
                break
        return time.perf_counter() - t0, plies

    lines = ["arena_bench base %dx%d vs base %dx%d (%s), %d games, max_plies %d"
             % (a.blocks, a.filters, a.blocks, a.filters, nets[0].tower_kernel, a.games, a.max_plies)]
    for engine in (False, True):                                  # warm-up: both paths, a few plies
        match(engine, 8, 1)
    own_stream(1)
    same, faster = True, True
    for r in range(a.repeats):
        th, hres, hhist, hresult = match(False, a.max_plies, 100 + r)
        te, eres, ehist, eresult = match(True, a.max_plies, 100 + r)
        plies = max(len(h) for h in hhist)
        ok = hhist == ehist and hresult == eresult and hres == eres
        same, faster = same and ok, faster and te < th
        done = sum(1 for x in hresult if x is not None)
        lines.append("  repeat %d host   %9.1f ms per match, %7.3f ms per ply (%d plies, %d games finished, avg batch %.1f)"
                     % (r, th * 1e3, th * 1e3 / plies, plies, done, hres.avg_batch_size))
        lines.append("  repeat %d engine %9.1f ms per match, %7.3f ms per ply, host / engine %.1f, same moves and results: %s"
                     % (r, te * 1e3, te * 1e3 / plies, th / te, ok))
        ts, sp = own_stream(100 + r)
        lines.append("  repeat %d engine, its own stream %7.1f ms per match, %7.3f ms per ply (%d plies)"
                     % (r, ts * 1e3, ts * 1e3 / sp, sp))
    lines.append("  engine (same uniforms as the host loop) faster in every repeat: %s; move lists equal in every repeat: %s"
                 % (faster, same))
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    assert same, "the engine arena and the host loop played different moves"
    return 0


if __name__ == "__main__":
    sys.exit(main())
