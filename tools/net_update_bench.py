#!/usr/bin/env python3
"""What it costs to hand the trainer's weights to self-play: the create path (Trainer.params(), 94 MB to
the host at 20x256, then AlphaZero(weights=...): az_net_create folds and packs on one host thread) against
the in-place device path (AlphaZero.update_from(trainer): az_net_update_from_trainer, kernels of
net_update.hip).  Wall time around each call; both return after their stream has been synchronised.

Per size one child process under its own time limit: one warm-up of each path, then alternated repeats,
and a check that the updated net's packed buffers equal the created one's byte for byte.

    python tools/net_update_bench.py [--repeats 3] [--out profiles/net_update_bench.txt]
"""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "alphazero-chess_amd"))

CASES = ("f32:20x256", "f32:10x128", "bf16:20x256", "fp8:20x256")
UPDATES = 20


def buffers(net, L):
    out = []
    for kind in L.PACKED_KINDS:
        for i in range(1 + 2 * net.blocks):
            b = net.packed(kind, i)
            if b is None:
                break
            out.append(b)
    return out


def child(case, repeats, device):
    import numpy as np
    import azchess as A
    import azchess._lib as L
    dtype, shape = case.split(":")
    blocks, filters = (int(v) for v in shape.split("x"))
    tr = A.Trainer(blocks, filters, max_batch=1, device=device, seed=7)
    net = A.AlphaZero(blocks, filters, weights=A.random_weights(blocks, filters, seed=8), dtype=dtype, device=device)

    def create():
        t0 = time.perf_counter()
        m = A.AlphaZero(blocks, filters, weights=tr.params(), dtype=dtype, device=device)
        return time.perf_counter() - t0, m

    def update(calls=UPDATES):
        """mean of `calls` updates back to back (one is well under a millisecond: too short a window)"""
        t0 = time.perf_counter()
        for _ in range(calls):
            net.update_from(tr)
        L.check(L.lib.az_device_synchronize(device))
        return (time.perf_counter() - t0) / calls

    _, ref = create()                                             # warm-up of both paths, and the parity check
    update()
    a, b = buffers(net, L), buffers(ref, L)
    same = len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))
    del ref
    print("net_update_bench %-5s %2dx%-3d (%s; %.1f MB of parameters) update == create: %s"
          % (dtype, blocks, filters, net.tower_kernel, tr.n * 4 / 1e6, same))
    best = {}
    for r in range(repeats):
        dt, m = create()
        del m
        best["create"] = min(best.get("create", dt), dt)
        print("  repeat %d create %10.2f ms" % (r, dt * 1e3))
        dt = update()
        best["update"] = min(best.get("update", dt), dt)
        print("  repeat %d update %10.3f ms (mean of %d calls)" % (r, dt * 1e3, UPDATES))
    print("  best create %.2f ms, best update %.3f ms, ratio %.0f"
          % (best["create"] * 1e3, best["update"] * 1e3, best["create"] / best["update"]))
    return 0 if same and best["update"] < best["create"] else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--timeout", type=int, default=180, help="seconds per size")
    ap.add_argument("--case", help="run one size in this process (dtype:BLOCKSxFILTERS)")
    ap.add_argument("--cases", nargs="*", default=list(CASES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "net_update_bench.txt"))
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
            lines.append("net_update_bench %s: no result within %d s; stopping" % (case, a.timeout))
            rc = 124
            break
        lines.append(p.stdout.rstrip())
        if p.returncode != 0:                                     # nothing more starts on the GPU after a failure
            lines.append("net_update_bench %s: exit status %d; stopping" % (case, p.returncode))
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
