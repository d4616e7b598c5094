"""The N > 1 rank path of bench.py with the REAL engine on a one-GPU box (--same-device maps every
rank to device 0 and skips the RCCL training leg).  It exercises the spawn, per-rank seeds, barrier,
max-over-ranks timing and counter sums with libaz doing the self-play -- not a scaling measurement
(no scaling curve has been measured: the driver had no 8-GPU node)."""
import pytest

from test_dist import _bench

pytestmark = pytest.mark.gpu


def test_bench_two_ranks_real_engine_on_one_gpu(require_gpu):
    G, S, K, steps = 32, 16, 8, 2     # the window ends mid-move: root visits non-zero
    rc, lines, err = _bench(["--gpus", "2", "--same-device", "--steps", str(steps), "--warmup", "1",
                             "--games", str(G), "--sims", str(S), "--sims-per-step", str(K), "--blocks", "2",
                             "--filters", "64", "--bf16-steps", "0", "--no-cpu-baseline", "--train-steps", "0",
                             "--games-leg", "0"], timeout=300)
    assert rc == 0, err[-3000:]
    assert len(lines) == 1
    r = lines[0]
    assert r["n_gpus"] == 2 and r["steps"] == steps and r["dtype"] == "f32"
    sims = r["value"] * r["ms_per_step"] * 1e-3 * steps
    assert abs(sims - 2 * G * K * steps) < 1e-6 * sims
    assert r["evals_per_sim"] > 0.5
    d = r["rank_root_digests"]
    assert len(d) == 2 and d[0] != d[1]          # distinct games per rank (per-rank seeds)
    assert "TEST MODE" in r["config"]["parallelism"]


def test_bench_dump_outputs_is_the_last_steps_roots_and_repeats(require_gpu, tmp_path):
    """--dump-outputs on a plain run: the roots after the last timed step (the window ends mid-move, so
    every root carries the move's simulations so far) as f32 / f64 arrays, bit-identical between two
    runs with the same arguments."""
    import numpy as np
    G, S, K, steps = 33, 16, 8, 1
    runs = []
    for d in ("a", "b"):
        rc, lines, err = _bench(["--gpus", "1", "--steps", str(steps), "--warmup", "0", "--games", str(G),
                                 "--sims", str(S), "--sims-per-step", str(K), "--blocks", "2", "--filters", "64",
                                 "--dump-outputs", str(tmp_path / d)], timeout=120)
        assert rc == 0 and len(lines) == 1, err[-3000:]
        assert lines[0]["full"] is False and lines[0]["training"] is None and lines[0]["cpu_baseline"] is None
        runs.append({n: np.load(tmp_path / d / (n + ".npy"))
                     for n in ("counters", "root_games", "root_improved", "root_moves", "root_visits", "root_depth")})
    a, b = runs
    assert a["root_improved"].shape == a["root_visits"].shape == (G, 4096) and a["root_depth"].shape == (G,)
    assert a["root_improved"].dtype == a["root_visits"].dtype == np.float32
    assert np.array_equal(a["root_games"], np.arange(G))
    tot = a["root_visits"].sum(1, keepdims=True)
    assert np.all(tot > 0) and np.all(tot <= K * steps)           # at most one root-child visit per simulation
    assert np.array_equal(a["root_improved"], a["root_visits"] / tot)     # k_readout: (float)N / (float)total
    assert G * K * steps in a["counters"]
    assert not a["root_moves"].any()
    for n in a:
        assert np.array_equal(a[n], b[n]), n


def test_bench_dump_outputs_at_a_move_boundary(require_gpu, tmp_path):
    """A window that ends with a completed move leaves re-rooted, unvisited roots: root_moves marks
    their legal moves (every game is one ply from the start position: black has 20) and no NaN is
    stored."""
    import numpy as np
    G, S, K, steps = 33, 16, 8, 2
    rc, lines, err = _bench(["--gpus", "1", "--steps", str(steps), "--warmup", "0", "--games", str(G),
                             "--sims", str(S), "--sims-per-step", str(K), "--blocks", "2", "--filters", "64",
                             "--dump-outputs", str(tmp_path)], timeout=120)
    assert rc == 0 and len(lines) == 1, err[-3000:]
    a = {n: np.load(tmp_path / (n + ".npy")) for n in ("counters", "root_improved", "root_moves", "root_visits")}
    assert not a["root_visits"].any() and not a["root_improved"].any()
    assert a["root_moves"].shape == (G, 4096) and set(np.unique(a["root_moves"])) == {0.0, 1.0}
    assert np.all(a["root_moves"].sum(1) == 20)
    assert G * K * steps in a["counters"] and G in a["counters"]         # simulations, moves of the window
