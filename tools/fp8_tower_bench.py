#!/usr/bin/env python3
"""MX-fp8 tower against the bf16 tower, alternated within one process on one MI355X.

Tower leg: the 20x256 net at 2048 rows per launch through az_net_forward_device (dense mode) on
device buffers: one warm-up of each dtype, then ROUNDS alternated rounds (fp8, bf16, fp8, ...) of
LAUNCHES launches each, every round bracketed by HIP events.  Search leg: BatchedSearch of 2048 games
x SIMS simulations from noised start-position roots for each dtype, FEN cache off so that every
expansion is a network row; one move as warm-up, then the wall time around a synchronised second move:
sims/s and evaluations per simulation.  The baseline is the bf16 tower of the same build in the same
run.  roofline.frac divides the residual tower's algorithmic FLOPs by the dense peak of the matrix
path: 5 PF for the block-scaled fp8 MFMA, 2.5 PF for bf16.  The shader clock is read (not set) from
sysfs around every round.

    python tools/fp8_tower_bench.py [--out profiles/fp8_tower_bench.txt]
"""
import argparse
import glob
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "alphazero-chess_amd"))

import numpy as np  # noqa: E402

import azchess as A  # noqa: E402
from azchess import _lib as L  # noqa: E402
from azchess.hiprt import Hip  # noqa: E402

PEAK_TFLOPS = {"fp8": 5000.0, "bf16": 2500.0}


def sclk_mhz():
    """current shader clock of card 0 from sysfs (the starred level), or None"""
    for path in sorted(glob.glob("/sys/class/drm/card*/device/pp_dpm_sclk")):
        try:
            for line in open(path):
                if "*" in line:
                    return int(line.split(":")[1].strip().lower().replace("mhz", "").replace("*", "").strip())
        except (OSError, ValueError, IndexError):
            pass
    return None


def tower_flop_per_row(blocks, filters):
    return 2.0 * 64.0 * (171.0 * filters + 18.0 * blocks * float(filters) * filters)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=20)
    ap.add_argument("--filters", type=int, default=256)
    ap.add_argument("--rows", type=int, default=2048)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--games", type=int, default=2048)
    ap.add_argument("--sims", type=int, default=48)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fp8_tower_bench.txt"))
    a = ap.parse_args()
    assert a.rounds >= 3
    hip = Hip()
    w = A.random_weights(a.blocks, a.filters, seed=42)
    nets = {d: A.AlphaZero(a.blocks, a.filters, weights=w, dtype=d) for d in ("fp8", "bf16")}
    planes = np.concatenate([A.to_tensor(A.Position.startpos())] * a.rows).reshape(a.rows, 19 * 64)
    d_in = hip.upload(np.ascontiguousarray(planes, np.float32))
    d_pol, d_val = hip.malloc(a.rows * 4096 * 4), hip.malloc(a.rows * 4)
    stream = hip.stream()

    def launch(dtype, n):
        for _ in range(n):
            L.check(L.lib.az_net_forward_device(nets[dtype]._h, d_in, a.rows, d_pol, d_val, stream))

    out = {d: {} for d in nets}
    for d in nets:                                        # warm-up, and the outputs for the record
        launch(d, 3)
        L.check(L.lib.az_device_synchronize(0))
        out[d]["value0"] = float(hip.download(d_val, np.zeros(a.rows, np.float32))[0])
    rounds = {d: [] for d in nets}
    clocks = {d: [] for d in nets}
    for _ in range(a.rounds):
        for d in ("fp8", "bf16"):
            e0, e1 = hip.event(), hip.event()
            hip.record(e0, stream)
            launch(d, a.launches)
            mid = sclk_mhz()
            hip.record(e1, stream)
            rounds[d].append(hip.elapsed_ms(e0, e1) / a.launches)
            clocks[d].append(mid)
    flop = tower_flop_per_row(a.blocks, a.filters) * a.rows
    res = {"config": {"blocks": a.blocks, "filters": a.filters, "rows": a.rows, "rounds": a.rounds, "launches": a.launches},
           "tower": {}, "search": {}}
    for d in nets:
        ms = float(np.median(rounds[d]))
        tf = flop / (ms * 1e-3) / 1e12
        res["tower"][d] = {"kernel": nets[d].tower_kernel, "ms_per_launch_rounds": [round(x, 4) for x in rounds[d]],
                           "ms_per_launch": round(ms, 4), "rows_per_s": round(a.rows / (ms * 1e-3)),
                           "sclk_mhz_during_rounds": clocks[d], "value_row0": out[d]["value0"],
                           "roofline": {"achieved_tflops": round(tf, 1), "peak_tflops": PEAK_TFLOPS[d],
                                        "frac": round(tf / PEAK_TFLOPS[d], 4)}}
    res["tower"]["fp8_over_bf16_speed"] = round(res["tower"]["bf16"]["ms_per_launch"] / res["tower"]["fp8"]["ms_per_launch"], 4)
    for d in nets:
        s = A.BatchedSearch(nets[d], games=a.games, sims=a.sims, seed=1, cache_capacity=0)
        s.set_roots([[]] * a.games, apply_noise=True)
        s.run()                                           # warm-up move
        s.set_roots([[]] * a.games, apply_noise=True)
        L.check(L.lib.az_device_synchronize(0))
        st0 = s.stats()
        t0 = time.perf_counter()
        s.run()
        L.check(L.lib.az_device_synchronize(0))
        dt = time.perf_counter() - t0
        st = s.stats()
        sims, evals = st["sims"] - st0["sims"], st["evals"] - st0["evals"]
        res["search"][d] = {"games": a.games, "sims": a.sims, "seconds": round(dt, 4), "sims_per_s": round(sims / dt),
                            "evals_per_sim": round(evals / max(sims, 1), 4), "persistent_kernel": bool(s.persistent),
                            "sclk_mhz_after": sclk_mhz()}
    res["search"]["fp8_over_bf16_speed"] = round(res["search"]["fp8"]["sims_per_s"] / res["search"]["bf16"]["sims_per_s"], 4)
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("# python tools/fp8_tower_bench.py (one MI355X; fp8 and bf16 alternated in one process)\n")
        f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
