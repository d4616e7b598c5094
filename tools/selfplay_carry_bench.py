#!/usr/bin/env python3
"""Self-play across weight updates, measured: the self-play phases of a three-iteration train() loop in
one process (10x128 f32, 256 slots, 64 simulations, train()'s search settings), the phases separated by
an in-place model.update(weights) with differently seeded random weights.  Two legs:

  lockstep  train()'s default form: per phase a fresh SelfPlay(continuous=False) played until its last
            game ends (games whose slot has finished leave the batch);
  carried   train(carry_games=True)'s form: one continuous SelfPlay for all phases, a phase ends once
            `slots` more games have finished, SelfPlay.adopt() carries the games in flight over the
            update.

Wall time around each phase (every step ends with a synchronised drain).  Per leg and phase: wall time,
EpisodeSteps drained per second, simulations per second, network rows per simulation step launched (every
move step launches `sims` of them, however many slots are still live) and the share of slots live over
the phase's move steps, and the adoption's own time.  The repeats of the two legs are interleaved.

    python tools/selfplay_carry_bench.py [--repeats 3] [--out profiles/selfplay_carry_bench.txt]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "alphazero-chess_amd"))

PHASES = 3


def delta(a, b):
    return {k: b[k] - a[k] for k in ("sims", "evals", "moves", "games_finished")}


def row(leg, repeat, phase, wall, steps, d, a, move_steps, adopt_s=None):
    launched = max(move_steps * a.sims, 1)                 # simulation steps launched in the phase
    return dict(leg=leg, repeat=repeat, phase=phase, wall=wall, steps=steps, steps_s=steps / wall,
                sims_s=d["sims"] / wall, batch=d["evals"] / launched, live=d["sims"] / (launched * a.slots),
                games=d["games_finished"], move_steps=move_steps, adopt_s=adopt_s)


def lockstep(A, model, weights, a, repeat, emit):
    for phase in range(PHASES):
        if phase:
            model.update(weights[phase])
        t0 = time.perf_counter()
        sp = A.SelfPlay(model, games=a.slots, sims=a.sims, device=a.device, continuous=False,
                        seed=a.seed + 7919 * phase)
        sp.reset()
        steps = move_steps = 0
        while True:
            _, active = sp.step()
            move_steps += 1
            steps += len(sp.drain_raw())
            if active == 0:
                break
        wall = time.perf_counter() - t0
        z = dict(sims=0, evals=0, moves=0, games_finished=0)
        emit(row("lockstep", repeat, phase, wall, steps, delta(z, sp.search.stats()), a, move_steps))
        del sp


def carried(A, model, weights, a, repeat, emit):
    sp = None
    for phase in range(PHASES):
        adopt_s = None
        if phase:
            model.update(weights[phase])
        t0 = time.perf_counter()
        if sp is None:
            sp = A.SelfPlay(model, games=a.slots, sims=a.sims, device=a.device, continuous=True, seed=a.seed)
            sp.reset()
        else:
            sp.adopt()
            adopt_s = time.perf_counter() - t0
        s0 = sp.search.stats()
        steps = done = move_steps = 0
        while done < a.slots:
            fin, _ = sp.step()
            move_steps += 1
            done += fin
            steps += len(sp.drain_raw())
        wall = time.perf_counter() - t0
        emit(row("carried", repeat, phase, wall, steps, delta(s0, sp.search.stats()), a, move_steps, adopt_s))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--blocks", type=int, default=10)
    ap.add_argument("--filters", type=int, default=128)
    ap.add_argument("--slots", type=int, default=256)
    ap.add_argument("--sims", type=int, default=64)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "selfplay_carry_bench.txt"))
    a = ap.parse_args()
    import azchess as A
    weights = [A.random_weights(a.blocks, a.filters, seed=100 + p) for p in range(PHASES)]
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    rows = []

    def emit(r):
        rows.append(r)
        say("  %-8s repeat %d phase %d: %6.2f s, %3d move steps, %3d games, %6d EpisodeSteps = %7.1f /s, %7.0f sims/s, "
            "%5.1f rows per simulation step, slots live %4.1f %%%s"
            % (r["leg"], r["repeat"], r["phase"], r["wall"], r["move_steps"], r["games"], r["steps"], r["steps_s"],
               r["sims_s"], r["batch"], 100 * r["live"],
               "" if r["adopt_s"] is None else ", adopt %.2f ms" % (r["adopt_s"] * 1e3)))

    model = A.AlphaZero(a.blocks, a.filters, weights=weights[0], dtype="f32", device=a.device)
    say("selfplay_carry_bench %dx%d f32 (%s), %d slots, %d simulations, %d phases, %d repeats"
        % (a.blocks, a.filters, model.tower_kernel, a.slots, a.sims, PHASES, a.repeats))
    for repeat in range(a.repeats):
        for leg in (lockstep, carried):
            model.update(weights[0])
            leg(A, model, weights, a, repeat, emit)
    wins = 0
    for repeat in range(a.repeats):
        tot = {}
        for leg in ("lockstep", "carried"):
            rs = [r for r in rows if r["leg"] == leg and r["repeat"] == repeat]
            tot[leg] = sum(r["steps"] for r in rs) / sum(r["wall"] for r in rs)
        wins += tot["carried"] > tot["lockstep"]
        say("  repeat %d, all phases: lockstep %.1f EpisodeSteps/s, carried %.1f (x%.2f)"
            % (repeat, tot["lockstep"], tot["carried"], tot["carried"] / tot["lockstep"]))
    say("  carried drains more EpisodeSteps per second than lockstep in %d of %d repeats" % (wins, a.repeats))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
