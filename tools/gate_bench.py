#!/usr/bin/env python3
"""What the model gate of train(gate=True) costs per iteration: the trainer's snapshot / restore /
set_params (device-to-device or host-to-device copies of the flat parameters on the trainer's stream), and
one gated iteration's tail -- the candidate net refreshed from the trainer, the 256-game base-vs-base match
in the engine arena, the restore of a rejected candidate -- beside the same iteration's 40 training steps
on 512-position batches (Trainer.step on host arrays, as train() feeds them without device_replay).  Wall
time around each call; every call returns with its stream idle.

Per size one child process under its own time limit: one warm-up of everything, then the repeats.

    python tools/gate_bench.py [--repeats 3] [--out profiles/gate_bench.txt]
"""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "alphazero-chess_amd"))

CASES = ("10x128", "20x256")
COPIES = 20
STEPS, BATCH, GAMES = 40, 512, 256


def child(case, repeats, device):
    import numpy as np
    import azchess as A
    from azchess.training import gate_seed
    blocks, filters = (int(v) for v in case.split("x"))
    tr = A.Trainer(blocks, filters, max_batch=BATCH, device=device, seed=7)
    model = tr.model("f32")
    candidate = tr.model("f32")
    host = A.random_weights(blocks, filters, seed=8)
    rng = np.random.default_rng(1)
    planes = (rng.random((BATCH, 19 * 64), dtype=np.float32) < 0.1).astype(np.float32)
    pol = rng.random((BATCH, 4096), dtype=np.float32) * (rng.random((BATCH, 4096), dtype=np.float32) < 0.01)
    pol[:, 0] += 1e-3
    pol /= pol.sum(1, keepdims=True, dtype=np.float32)
    val = rng.uniform(-1, 1, BATCH).astype(np.float32)

    def mean_of(fn, calls=COPIES):
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        return (time.perf_counter() - t0) / calls

    def train_phase():
        t0 = time.perf_counter()
        for _ in range(STEPS):
            tr.step(planes, pol, val, 1e-3)
        return time.perf_counter() - t0

    def tail(it):
        t0 = time.perf_counter()
        tr.model("f32", into=candidate)
        t1 = time.perf_counter()
        r = A.evaluate(A.Player.base(candidate), A.Player.base(model), games=GAMES, engine=True,
                       seed=gate_seed(7, it), device=device)
        t2 = time.perf_counter()
        tr.restore()
        t3 = time.perf_counter()
        return t1 - t0, t2 - t1, t3 - t2, r.winrate

    print("gate_bench %2dx%-3d (%s; %.1f MB of parameters)" % (blocks, filters, model.tower_kernel, tr.n * 4 / 1e6))
    tr.snapshot()                                                  # warm-up: the snapshot buffer, every kernel, the arena
    tr.set_params(host)
    tr.step(planes, pol, val, 1e-3)
    tail(0)
    best = {}
    for r in range(repeats):
        tr.snapshot()
        got = {"snapshot": mean_of(tr.snapshot), "train": train_phase()}
        got["refresh"], got["match"], got["restore1"], winrate = tail(r + 1)
        got["restore"] = mean_of(tr.restore)
        got["set_params"] = mean_of(lambda: tr.set_params(host))
        got["tail"] = got["refresh"] + got["match"] + got["restore1"]
        for k, v in got.items():
            best[k] = min(best.get(k, v), v)
        print("  repeat %d snapshot %.3f ms, restore %.3f ms, set_params (host) %.3f ms (means of %d calls); "
              "%d steps of %d: %.3f s; tail: refresh %.3f ms + %d-game match %.3f s (winrate %.3f) + restore %.3f ms"
              % (r, got["snapshot"] * 1e3, got["restore"] * 1e3, got["set_params"] * 1e3, COPIES, STEPS, BATCH,
                 got["train"], got["refresh"] * 1e3, GAMES, got["match"], winrate, got["restore1"] * 1e3))
    print("  best snapshot %.3f ms, restore %.3f ms, set_params (host) %.3f ms; training phase %.3f s, gate tail %.3f s "
          "(%.0f %% of the training phase; the copies are %.3f %% of it)"
          % (best["snapshot"] * 1e3, best["restore"] * 1e3, best["set_params"] * 1e3, best["train"], best["tail"],
             100 * best["tail"] / best["train"], 100 * (best["snapshot"] + best["restore"]) / best["train"]))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per size")
    ap.add_argument("--case", help="run one size in this process (BLOCKSxFILTERS)")
    ap.add_argument("--cases", nargs="*", default=list(CASES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gate_bench.txt"))
    a = ap.parse_args()
    if a.case:
        return child(a.case, a.repeats, a.device)
    lines, rc = [], 0
    for case in a.cases:
        cmd = [sys.executable, os.path.abspath(__file__), "--case", case, "--repeats", str(a.repeats),
               "--device", str(a.device)]
        try:
            p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=a.timeout)
        except subprocess.TimeoutExpired:
            lines.append("gate_bench %s: no result within %d s; stopping" % (case, a.timeout))
            rc = 124
            break
        lines.append(p.stdout.rstrip())
        if p.returncode != 0:                                     # nothing more starts on the GPU after a failure
            lines.append("gate_bench %s: exit status %d; stopping" % (case, p.returncode))
            rc = p.returncode
            break
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
