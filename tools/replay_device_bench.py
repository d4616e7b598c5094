#!/usr/bin/env python3
"""Host replay path against the device-backed buffer, on one MI355X, in one process.

Buffers of --entries unique positions (seeded random playouts; drained-shape az_episode_step records:
the legal indices in generator order with a visit count each), a 20x256 trainer.

Leg 1: --steps steps of  sample_arrays(512) + step  against  step_replay(512).
Leg 2: the same draw of 512, training rows [0, 64) on a max_batch-64 trainer: a world-8 rank's step.
Leg 3: add_many of --adds drained-shape steps into a fresh host buffer and a fresh device buffer.

One warm-up, then --repeats alternated repeats of the host and the device path; wall time around a block
that ends in a device synchronise.  The host path is the step loop of train() as it stands.  Also the
host resident memory each buffer adds.  The parameters of the two trainers of a leg are compared at
the end (they took the same steps): equal bit for bit.

    python tools/replay_device_bench.py [--out profiles/replay_device_bench.txt]
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "alphazero-chess_amd"))

import azchess as A  # noqa: E402
from azchess import _lib as L  # noqa: E402
from azchess import memory as M  # noqa: E402
from azchess.memory import ReplayBuffer  # noqa: E402
from azchess.training import Trainer, get_cyclical_lr  # noqa: E402


def rss_mb():
    with open("/proc/self/statm") as f:
        return int(f.read().split()[1]) * os.sysconf("SC_PAGE_SIZE") / 2 ** 20


def sync(device=0):
    L.check(L.lib.az_device_synchronize(device))


def unique_steps(n, seed, plies=80):
    """n az_episode_step records of n distinct positions from random playouts, as one ctypes array."""
    rng = np.random.default_rng(seed)
    raw = np.zeros((n, M._STEP_SIZE), np.uint8)
    seen = set()
    k = 0
    while k < n:
        gs = A.GameState()
        for _ in range(plies):
            pos = gs.position
            idx = pos.legal_indices()
            if len(idx) == 0:
                break
            fen = pos.fen()
            if fen not in seen:
                seen.add(fen)
                st = L.AzEpisodeStep()
                st.state = pos._p
                st.final_value = float(rng.uniform(-1, 1))
                st.nvis = len(idx)
                row = np.frombuffer(st, np.uint8).copy()
                row[M._IDX:M._IDX + 2 * len(idx)] = np.asarray(idx, "<u2").view(np.uint8)
                row[M._CNT:M._CNT + 2 * len(idx)] = rng.integers(0, 60, len(idx)).astype("<u2").view(np.uint8)
                raw[k] = row
                k += 1
                if k == n:
                    break
            if int(A.play_move(gs, int(rng.choice(idx)))) != 0:
                break
    return raw


def as_steps(raw):
    return (L.AzEpisodeStep * raw.shape[0]).from_buffer_copy(raw.tobytes())


def host_loop(trainer, replay, steps, batch, lo, hi, lr, seed0):
    """train()'s step loop on the host path; returns (wall s, s in sample_arrays, s in step)."""
    sync()
    ts = tt = 0.0
    t0 = time.perf_counter()
    for b in range(steps):
        a = time.perf_counter()
        planes, pol, val, _ = replay.sample_arrays(batch, seed=seed0 + b)
        c = time.perf_counter()
        trainer.step(planes[lo:hi], pol[lo:hi], val[lo:hi], lr)
        ts += c - a
        tt += time.perf_counter() - c
    sync()
    return time.perf_counter() - t0, ts, tt


def device_loop(trainer, replay, steps, batch, lo, hi, lr, seed0):
    sync()
    t0 = time.perf_counter()
    for b in range(steps):
        trainer.step_replay(replay, batch, seed0 + b, lr, lo, hi)
    sync()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--entries", type=int, default=20000)      # MIN_REPLAY_SIZE
    ap.add_argument("--steps", type=int, default=40)           # NUM_TRAIN_STEPS
    ap.add_argument("--adds", type=int, default=50000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--blocks", type=int, default=20)
    ap.add_argument("--filters", type=int, default=256)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--shard", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "replay_device_bench.txt"))
    a = ap.parse_args()
    n = C.c_int(0)
    L.lib.az_device_count(C.byref(n))
    if n.value < 1:
        sys.exit("replay_device_bench: no GPU (this measurement has no host fall-back)")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    raw = unique_steps(a.entries, seed=1)
    steps = as_steps(raw)
    # the HIP runtime, libaz's code objects and the add staging are resident before anything is measured
    tiny = ReplayBuffer(4, device=0)
    tiny.add_many(as_steps(raw[:min(300, a.entries)]))
    tiny.sample_arrays(4, 0)
    del tiny
    sync()
    r0 = rss_mb()
    host = ReplayBuffer(a.entries)
    new_h = host.add_many(steps)
    r1 = rss_mb()
    dev = ReplayBuffer(a.entries, device=0)
    new_d = dev.add_many(steps)
    r2 = rss_mb()
    assert new_h == new_d == a.entries == len(host) == len(dev)
    say("replay_device_bench %dx%d, %d entries: host buffer + %.0f MB resident on the host, device buffer + %.0f MB "
        "(its rows: %.0f MB of HBM)" % (a.blocks, a.filters, a.entries, r1 - r0, r2 - r1, a.entries * 16468 / 2 ** 20))
    lr = get_cyclical_lr(0)
    w = A.random_weights(a.blocks, a.filters, seed=3)
    for leg, (maxb, lo, hi) in enumerate([(a.batch, 0, a.batch), (a.shard, 0, a.shard)], 1):
        th, td = Trainer(a.blocks, a.filters, w, max_batch=maxb), Trainer(a.blocks, a.filters, w, max_batch=maxb)
        say("leg %d: %d steps, draw %d, train rows [%d, %d)" % (leg, a.steps, a.batch, lo, hi))
        host_loop(th, host, 3, a.batch, lo, hi, lr, 10 ** 6)             # warm-up, the same steps on both
        device_loop(td, dev, 3, a.batch, lo, hi, lr, 10 ** 6)
        faster = True
        for rep in range(a.repeats):
            s0 = 1000 * rep
            wh, ts, tt = host_loop(th, host, a.steps, a.batch, lo, hi, lr, s0)
            wd = device_loop(td, dev, a.steps, a.batch, lo, hi, lr, s0)
            faster = faster and wd < wh
            say("  repeat %d host %8.3f ms/step (sample_arrays %7.3f + step %7.3f)   device %8.3f ms/step   ratio %.2f"
                % (rep, 1e3 * wh / a.steps, 1e3 * ts / a.steps, 1e3 * tt / a.steps, 1e3 * wd / a.steps, wh / wd))
        say("  device path faster in every repeat: %s; parameters equal bit for bit: %s"
            % (faster, th.params().tobytes() == td.params().tobytes()))
        del th, td
    rng = np.random.default_rng(9)
    many = as_steps(raw[rng.integers(0, a.entries, a.adds)])
    say("leg 3: add_many of %d steps over %d positions into an empty buffer" % (a.adds, a.entries))
    for rep in range(-1, a.repeats):                                     # -1: warm-up
        hb = ReplayBuffer(a.entries)
        t0 = time.perf_counter()
        nh = hb.add_many(many)
        t1 = time.perf_counter()
        del hb
        db = ReplayBuffer(a.entries, device=0)
        sync()
        t2 = time.perf_counter()
        nd = db.add_many(many)
        sync()
        t3 = time.perf_counter()
        del db
        assert nh == nd
        if rep >= 0:
            say("  repeat %d host %8.1f ms (%.2f us/step)   device %8.1f ms (%.2f us/step)   ratio %.2f"
                % (rep, 1e3 * (t1 - t0), 1e6 * (t1 - t0) / a.adds, 1e3 * (t3 - t2), 1e6 * (t3 - t2) / a.adds,
                   (t1 - t0) / (t3 - t2)))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
