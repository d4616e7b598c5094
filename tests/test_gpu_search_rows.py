"""Search-mode evaluations of every network path against the dense forward of the same net, bit for bit.

Every path has a dense kernel (planes in, 4096 priors and a value out) and a separately compiled search kernel
(to_tensor staged from the leaf's stored position, its row found through row_game / row_node, priors written at
the node's legal indices, an eval-log record appended).  Both do the same arithmetic on the same planes, so a
logged row equals the dense forward of that position at the node's legal indices exactly -- whatever the
kernel's numerics are.  The oracle's replay cannot see a wrong evaluation; this can.

For each entry of the dispatch matrix (tests/searchrows.py PATHS; the kernel that runs is asserted) a
24-simulation search runs from 17 roots that reach the plane and edge-count corners by themselves
(tests/test_searchrows.py; two of them are there twice, in other batch rows), with the evaluation log on.  The position behind every logged key is found by the
oracle alone (searchrows.closure), its planes are the oracle's to_tensor, and one dense forward of the same net
object gives the rows to compare with.  The dense rows, which have never seen such planes, are also held to the
dtype's tolerance against float64 (netcases.forward64; fp8: tests/mx8_ref.py), one ROWS line per case.

Modes: the step kernels (AZ_PERSIST=0), the persistent per-game kernel where it exists (the same rows as the
step mode, bit for bit), leaf-parallel waves of 4, and root noise (the log holds the un-noised rows)."""
import time

import numpy as np
import pytest

import azchess as A
import mx8_ref as R
import netcases as N
import oracle as O
import searchrows as S

pytestmark = pytest.mark.gpu

SIMS = 24
GAMES = len(S.ROOTS)
LOG_CAP = 4096            # rows; 64 priors per row on average: 17 x 25 rows of at most 218 priors fit many times
_logs = {}                # (path id, mode) -> {key: (value, idx, priors)} of a checked run
_ref64 = {}               # filters -> {key: (policy float64 [4096], value float64)}
_weights = {}


def weights(filters):
    if filters not in _weights:
        _weights[filters] = A.random_weights(S.BLOCKS, filters, seed=42)
    return _weights[filters]


def make_net(monkeypatch, pid):
    """the net of a matrix entry, created under its environment; which kernel evaluates it is asserted"""
    _id, dtype, filters, env, kernel, _pers, form = S.PATH[pid]
    for k in S.NET_ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    net = A.AlphaZero(S.BLOCKS, filters, weights=weights(filters), dtype=dtype)
    assert net.tower_kernel == kernel, (pid, net.tower_kernel)
    if form is not None:
        got = (net.wino_streamed_points, net.wino_accumulators, net.wino_v_rows, net.wino_boards)
        assert got == form, (pid, got)
    return net


def reference(filters, keys, planes):
    """float64 policy and value rows of the positions, computed once per (net, position)"""
    have = _ref64.setdefault(filters, {})
    new = [i for i, k in enumerate(keys) if k not in have]
    for a in range(0, len(new), 64):
        rows = new[a:a + 64]
        pol, val = N.forward64(S.BLOCKS, filters, weights(filters), planes[rows])
        for j, i in enumerate(rows):
            have[keys[i]] = (pol[j], val[j])
    return np.stack([have[k][0] for k in keys]), np.array([have[k][1] for k in keys])


def check_dense(pid, mode, dtype, filters, keys, planes, pol, val):
    """the dense rows against float64 within the dtype's tolerance; prints the share of it they use"""
    rpol, rval = reference(filters, keys, planes)
    assert np.isfinite(pol).all() and np.isfinite(val).all()
    t = R.TOL_FP8 if dtype == "fp8" else N.TOL[dtype]
    ev = float(np.abs(val - rval).max()) / t["v"]
    ep = float((np.abs(pol - rpol) / (t["prel"] * rpol + t["pabs"])).max())
    tv = float(np.max(0.5 * np.abs(pol - rpol).sum(1)))
    print("ROWS %-16s %-10s %dx%-3d %4d positions: dense rows against float64, error / bound: value %.3f policy %.3f "
          "(total variation %.2e)" % (pid, mode, S.BLOCKS, filters, len(keys), ev, ep, tv))
    assert ev <= 1.0, "value error %.3f x its bound %g" % (ev, t["v"])
    assert ep <= 1.0, "policy error %.3f x its bound %g p + %g" % (ep, t["prel"], t["pabs"])
    if dtype == "fp8":
        assert tv <= t["tv"]
    if dtype == "bf16":
        assert tv <= 2e-2         # netcases.check_tolerance


def run_case(monkeypatch, pid, mode):
    """One search of a path in a mode ("step", "persistent", "leaves", "noise") with every logged row checked
    against the dense forward; returns {key: (value, idx, priors)}."""
    if (pid, mode) in _logs:
        return _logs[pid, mode]
    t0 = time.perf_counter()
    _id, dtype, filters, _env, _kernel, pers, _form = S.PATH[pid]
    net = make_net(monkeypatch, pid)
    monkeypatch.setenv("AZ_PERSIST", "1" if mode == "persistent" else "0")
    noise = mode == "noise"
    s = A.BatchedSearch(net, games=GAMES, sims=SIMS, seed=11, noise=noise, cache_capacity=0, record_evals=True,
                        eval_log_cap=LOG_CAP, leaves=4 if mode == "leaves" else 1)
    assert s.persistent == (mode == "persistent"), (pid, mode)
    assert mode != "persistent" or pers
    assert s.leaves == (4 if mode == "leaves" else 1)
    s.set_roots([h for _, h in S.ROOTS], apply_noise=noise, start=[A.Position.from_fen(f) for f, _ in S.ROOTS])
    _imp, vis, _dep = s.run()
    assert np.all(vis.sum(1) == SIMS)
    keys, vals, off, idx, pri = s.eval_log()
    st = s.stats()
    assert st["overflow"] == 0
    assert len(keys) == st["evals"] + GAMES, (len(keys), st["evals"])
    assert len(keys) < LOG_CAP and len(pri) < 64 * LOG_CAP and len(off) == len(keys) + 1 and off[-1] == len(pri)
    assert st["terminal_leaves"] > 0 and len(keys) < GAMES * (SIMS + 1)      # steps with fewer rows than games

    pos = S.closure(S.ROOTS, keys)                   # raises if a logged key is not reached
    order = sorted(pos)
    assert set(order) == set(int(k) for k in keys)
    for fen, hist in S.ROOTS:                        # every root's evaluation is in the log
        assert int(O.fen_key(S.root_position(fen, hist))) in pos, fen
    planes = S.oracle_planes([pos[k] for k in order])
    pol, val = net.forward(planes)
    row = {k: i for i, k in enumerate(order)}
    legal = {k: set(O.legal_indices(pos[k]).tolist()) for k in order}

    log, bad = {}, []
    for r in range(len(keys)):
        k = int(keys[r])
        i = row[k]
        ii, pr = idx[off[r]:off[r + 1]], pri[off[r]:off[r + 1]]
        assert set(ii.tolist()) == legal[k], (pid, mode, r, O.to_fen(pos[k]))
        assert len(ii) == len(legal[k]), (pid, mode, r, O.to_fen(pos[k]))
        if not (vals[r] == val[i] and np.array_equal(pr, pol[i][ii])):
            bad.append((r, O.to_fen(pos[k]), float(vals[r]), float(val[i]), float(np.abs(pr - pol[i][ii]).max())))
        prev = log.setdefault(k, (np.float32(vals[r]), ii.copy(), pr.copy()))      # logged twice: the same bits
        assert prev[0] == vals[r] and np.array_equal(prev[1], ii) and np.array_equal(prev[2], pr), (pid, mode, r)
    assert not bad, "%s %s: %d of %d logged rows differ from the dense forward, e.g. %s" % (
        pid, mode, len(bad), len(keys), bad[:3])
    if not noise:          # the two roots that are there twice search alike: their positions were logged twice
        assert len(keys) >= len(order) + 2 * len(S.TWICE), (len(keys), len(order))
    edges = [len(v) for v in legal.values()]
    assert max(edges) == 218 and min(edges) == 1
    check_dense(pid, mode, dtype, filters, order, planes, pol, val)
    print("ROWS %-16s %-10s %s: %d rows, %d positions, %d shared leaves, %.2f s"
          % (pid, mode, net.tower_kernel.split(" ")[0], len(keys), len(order), s.shared_leaves, time.perf_counter() - t0))
    _logs[pid, mode] = log
    return log


@pytest.mark.parametrize("pid", [p[0] for p in S.PATHS])
def test_step_mode_rows_equal_the_dense_forward(require_gpu, monkeypatch, pid):
    """every path through k_step + its search kernel (the unfused paths: encode_rows_kernel, the per-layer
    convs, heads_kernel<F, T, true>)"""
    run_case(monkeypatch, pid, "step")


@pytest.mark.parametrize("pid", [p[0] for p in S.PATHS if p[5]])
def test_persistent_rows_equal_the_dense_forward_and_the_step_mode(require_gpu, monkeypatch, pid):
    """every path with a persistent per-game kernel (k_sims32w): the hard assertion, and the same set of rows
    with the same bits as the step mode of that path"""
    got = run_case(monkeypatch, pid, "persistent")
    want = run_case(monkeypatch, pid, "step")
    assert sorted(got) == sorted(want), (len(got), len(want))
    for k, (v, ii, pr) in want.items():
        v2, ii2, pr2 = got[k]
        assert v == v2 and np.array_equal(ii, ii2) and np.array_equal(pr, pr2), k


@pytest.mark.parametrize("pid", S.LEAF_PATHS)
def test_leaf_parallel_rows_equal_the_dense_forward(require_gpu, monkeypatch, pid):
    """waves of 4 leaves per game: several rows of a game in row_game / row_node, shared leaves"""
    run_case(monkeypatch, pid, "leaves")


@pytest.mark.parametrize("pid", S.NOISE_PATHS)
def test_noised_roots_log_the_network_rows(require_gpu, monkeypatch, pid):
    """Dirichlet noise changes a root's stored priors after its evaluation; the log holds the network's rows"""
    run_case(monkeypatch, pid, "noise")
