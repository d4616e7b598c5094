#!/usr/bin/env python3
"""What tree reuse (az_search_set_tree_reuse) does to continuous self-play: reuse off against
on in one process.

Per leg two SelfPlay handles on one net (continuous, noise on, FEN cache off), one with tree_reuse=True.  One
warm-up run of each, then alternated repeats; a run is reset() + a fixed number of moves, wall time around
it (every move ends in the driver's read-back of the finished move, a stream synchronise; a device
synchronise closes the block).  Reported per mode: moves per second (slots x moves / wall), network rows per
move, simulation steps per move (az_selfplay_run_sims(1) calls until the move is done, counted in the warm-up
run) and the carried
share (visits kept by re-roots / (slots x moves x sims)).  The two modes search differently, so they play
different games: this compares throughput, not results.

Legs (slots x sims x net):  A 2048 x 800 x 20x256   B 256 x 64 x 10x128   C 256 x 800 x 6x64 (off runs the
persistent per-game kernel there, on cannot: reported as it falls).

    python tools/treereuse_bench.py [--legs ABC] [--repeats 3] [--moves-a 3 --moves-b 24 --moves-c 6]
                                    [--out profiles/treereuse_bench.txt]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "alphazero-chess_amd"))

LEGS = {"A": (2048, 800, 20, 256), "B": (256, 64, 10, 128), "C": (256, 800, 6, 64)}


def emit(lines, text):
    lines.append(text)
    print(text, flush=True)


def run(A, sp, moves, count_steps):
    """reset + `moves` moves -> (seconds, rows, simulations, [steps per move] if counted, carried visits)"""
    import ctypes
    t0 = time.perf_counter()
    sp.reset()
    steps = []
    for _ in range(moves):
        if count_steps:
            steps.append(1)
            while not sp.run_sims(1)[2]:
                steps[-1] += 1
        else:
            sp.step()
        sp.drain_raw()
    A._lib.check(A._lib.lib.az_device_synchronize(ctypes.c_int(0)))
    dt = time.perf_counter() - t0
    st = sp.search.stats()
    return dt, st["evals"], st["sims"], steps, sp.reuse_stats()["carried_visits"]


def leg(A, name, moves, repeats, lines):
    slots, sims, blocks, filters = LEGS[name]
    net = A.AlphaZero(blocks, filters, weights=A.random_weights(blocks, filters, seed=42), dtype="f32")
    sps = {on: A.SelfPlay(net, games=slots, sims=sims, seed=7, continuous=True, cache_capacity=0, tree_reuse=on)
           for on in (False, True)}
    emit(lines, " %s: %d slots x %d sims x %dx%d f32 (random-init, seed 42), %d moves a run; persistent kernel: off %s, on %s"
         % (name, slots, sims, blocks, filters, moves, sps[False].search.persistent, sps[True].search.persistent))
    # the warm-up run counts the steps of each move (one az_selfplay_run_sims(1) call per step: the same
    # kernels as the timed form, not its host pattern); a game's first move has nothing to carry, so the
    # figure reported is the mean over the moves after it
    steps = {}
    for on in (False, True):
        per_move = run(A, sps[on], min(moves, 2 if name == "A" else 4), True)[3]
        steps[on] = sum(per_move[1:]) / max(len(per_move) - 1, 1)
    res = {False: [], True: []}
    for r in range(repeats):
        for on in (False, True):
            res[on].append(run(A, sps[on], moves, False))
    for on in (False, True):
        rates = [slots * moves / dt for dt, _, _, _, _ in res[on]]
        _, rows, nsims, _, carried = res[on][-1]
        emit(lines, "    reuse %-3s  moves/s %s  (median %.1f)  rows/move %.1f  sims/move %.1f  steps/move after the first %.1f  carried share %.1f %%"
             % ("on" if on else "off", " ".join("%.1f" % x for x in rates), sorted(rates)[len(rates) // 2],
                rows / (slots * moves), nsims / (slots * moves), steps[on], 100.0 * carried / (slots * moves * sims)))
    off, on = (sorted(slots * moves / r[0] for r in res[k])[repeats // 2] for k in (False, True))
    emit(lines, "    on / off, median moves/s: %.3f" % (on / off))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="ABC")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--moves-a", type=int, default=3)
    ap.add_argument("--moves-b", type=int, default=24)
    ap.add_argument("--moves-c", type=int, default=6)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "treereuse_bench.txt"))
    args = ap.parse_args()
    import azchess as A
    lines = []
    emit(lines, "tree reuse off / on, continuous self-play from the startpos, %d alternated repeats after one warm-up" % args.repeats)
    for name in args.legs:
        leg(A, name, {"A": args.moves_a, "B": args.moves_b, "C": args.moves_c}[name], args.repeats, lines)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
