"""The search under sharp evaluations (tests/sharpcases.py: one-hot, all-zero, uniform, subnormal, NaN / inf
priors; values at exactly 0, +-1 and NaN) against the numpy restatements tests/leafpar_ref.py and
tests/treereuse_ref.py, which tests/test_sharpcases.py checks against the C oracle.  Bar: BIT-EXACT visits,
improved policies (as uint32), depths, actions, results and counters.

The synthetic evaluator and random-initialised nets give near-flat priors, under which a tree stays 4 to 5
plies deep; a trained network's trees are dozens of plies deep.  What these cases reach that no other test
does: backup_game's / backup_game_k's loop over path levels 64 and up, paths of the length of the whole
search (PMAX = S + 2, S + 1 nodes of NMAX = S + 2), mates and third repetitions found far below the root and
re-selected as known-terminal leaves, reroot_keep_subtree on a chain across 64-node chunks, exact ties at the
maximum in both argmax paths (<= 64 and > 64 edges) below the root, the selection arithmetic on 0, subnormal,
+inf and NaN priors and on NaN scores, and waves of K leaves that all go down one edge.

The references and the conditions the cases rest on are computed and asserted in tests/test_sharpcases.py
(no GPU); its lines, as measured there:

deep line          hashed  start    sims 200 K 1: depth 191, 201 nodes, no terminal leaf
deep line          hashed  shuffle  sims 200 K 1: depth 200
deep line          hashed  wide     sims 200 K 1: depth 160, new_terminal 1, known_terminal 39, 13 wide nodes
deep mate          first   start    sims 200 K 1: depth 86, new_terminal 16, known_terminal 38, ties 117
deep leaf-parallel hashed  start    sims 400 K 4: depth 80, shared 224
deep leaf-parallel first   start    sims 600 K 8: depth 68, shared 441, new_terminal 14, known_terminal 14
in-tree repetition last    start    sims  64 K 1: the line ends 12 plies below the root (halfmove clock 12), depth 11,
                                                  known_terminal 52; every repeated position on the tree path
in-tree repetition last    lastline sims  64 K 1: the line ends 7 plies below the root, depth 6, known_terminal 57; the
                                                  repeated position once in the history, twice on the tree path
ties               uniform start    sims  64 K 1: depth 2, ties 105 (44 below the root)
ties               zeros   start    sims  64 K 1: depth 8, ties 109 (80 below the root)
wide nodes         zeros   wide     sims 200 K 1: depth 10, 90 wide nodes, ties 280 (177 at wide nodes)
wide nodes         nanmix  wide     sims 200 K 1: depth 12, 106 wide nodes, ties 402 (263 at wide nodes), inf taken 438,
                                                  fallback to the first edge 23
non-finite         nanmix  start    sims  64 K 1: depth 17, ties 191, inf taken 209
non-finite         nanmix  start    sims 200 K 1: depth 17, inf taken 610, fallback to the first edge 171
all NaN            allnan  start    sims  64 K 1: depth 62, every selection the first edge
tree reuse         hashed  start    160 sims x 4 plies: depth 151, every re-root carries 159 visits and keeps 160 nodes
tree reuse         nanmix  start    160 sims x 4 plies: kept 81 / 97 / 98
tree reuse         zeros   start    160 sims x 4 plies: kept 70 / 114 / 75
leaf-parallel      nanmix  wide     sims  64 K 8: depth 8, shared 53; allnan start K 4: depth 16, shared 48
in-engine net      gamma5+peaked 2x32 / 6x64, 200 sims, noise off: depth 9 / 10 through the C oracle's RefNet (all these
                                                  weights give); the three noised roots of the test: 7, 6, 5 / 7, 9, 10"""
import numpy as np
import pytest

import azchess as A
import netcases as N
import oracle as O
import sharpcases as S
import test_sharpcases as H
from test_gpu_leafpar import assert_matches, identity_holds
from test_gpu_search import compare_steps
from test_gpu_treereuse import assert_counters, assert_stepwise, drive

pytestmark = pytest.mark.gpu
F = np.float32
SEED = H.SEED


def run_search(family, sims, roots, noise, runs=1, **kw):
    """one handle, root g of `roots` its game g, the family through the callback evaluator -> (handle, the
    read-out of each of `runs` set_roots() + run())"""
    starts, hists = H.engine_roots(roots)
    s = A.BatchedSearch(None, games=len(roots), sims=sims, noise=noise, seed=SEED, evaluator=S.gpu_evaluator(family), **kw)
    outs = []
    for _ in range(runs):
        s.set_roots(hists, apply_noise=noise, start=starts)
        outs.append(s.run())
    return s, outs


def check_counters(s, refs, runs=1):
    """the handle's counters against the restatement's tallies (test_gpu_leafpar.identity_holds and the sums)"""
    known = runs * sum(r.counts["known_terminal"] for r in refs)
    st = identity_holds(s, known_terminal=known)
    assert st["sims"] == runs * sum(r.sims for r in refs), st
    assert st["evals"] + st["cache_hits"] == runs * sum(r.evals for r in refs), st
    assert st["terminal_leaves"] == runs * sum(r.counts["new_terminal"] for r in refs), st
    assert s.shared_leaves == runs * sum(r.shared for r in refs)
    assert st["max_nodes"] <= st["node_cap"] and st["max_edges"] <= st["edge_cap"], st
    return st


# ------------------------------------------------------------------ 1. stepwise, K = 1
@pytest.mark.parametrize("fused", ["1", "0"])
@pytest.mark.parametrize("name,noise", [(n, False) for n in H.STEP_CASES] + [(n, True) for n in H.NOISE_CASES])
def test_stepwise_bit_exact(require_gpu, monkeypatch, name, noise, fused):
    monkeypatch.setenv("AZ_FUSED_STEPS", fused)
    family, sims, roots = H.STEP_CASES[name]
    refs = H.step_refs(name, noise)
    s, outs = run_search(family, sims, roots, noise, cache_capacity=0)
    assert s.leaves == 1 and s.persistent is False
    assert_matches(outs[0], [r.out for r in refs])
    st = check_counters(s, refs)
    assert st["cache_hits"] == 0
    if name == "hashed" and not noise:                        # the chain: sims + 1 nodes of NMAX = sims + 2
        assert st["max_nodes"] == sims + 1 and st["node_cap"] == sims + 2, st


# ------------------------------------------------------------------ 2. leaf-parallel
@pytest.mark.parametrize("fused", ["1", "0"])
@pytest.mark.parametrize("name", sorted(H.LEAF_CASES))
def test_leaf_parallel_bit_exact(require_gpu, monkeypatch, name, fused):
    """hashed_k4 / first_k8: paths past 64 levels through select_game_k / backup_game_k with more than half
    the leaves shared; uniform, zeros, nanmix: virtual loss on exact ties and on non-finite edges; allnan_k4:
    every leaf of every wave takes the first edge"""
    monkeypatch.setenv("AZ_FUSED_STEPS", fused)
    family, sims, K, roots = H.LEAF_CASES[name]
    refs = H.leaf_refs(name)
    s, outs = run_search(family, sims, roots, False, cache_capacity=0, leaves=K)
    assert s.leaves == K
    assert_matches(outs[0], [r.out for r in refs])
    check_counters(s, refs)


# ------------------------------------------------------------------ 3. tree reuse
@pytest.mark.parametrize("fused", ["1", "0"])
@pytest.mark.parametrize("family", sorted(H.REUSE_CASES))
def test_tree_reuse_bit_exact(require_gpu, monkeypatch, family, fused):
    """hashed: every re-root keeps a chain of 160 nodes, each node's parent the one before it, over three
    64-node chunks; nanmix / zeros: part of the tree, with NaN scores and exact ties carried along"""
    monkeypatch.setenv("AZ_FUSED_STEPS", fused)
    refs, _ = H.reuse_refs(family)
    starts, hists = H.engine_roots(H.REUSE_CASES[family])
    s = A.BatchedSearch(None, games=len(hists), sims=H.REUSE_SIMS, noise=False, seed=SEED, cache_capacity=0,
                        tree_reuse=True, evaluator=S.gpu_evaluator(family))
    assert s.tree_reuse is True
    s.set_roots(hists, apply_noise=False, start=starts)
    assert_stepwise(drive(s, H.REUSE_PLIES, False), refs)
    st = assert_counters(s, refs, H.REUSE_PLIES)
    assert st["node_cap"] == H.REUSE_SIMS + 2
    if family == "hashed":
        assert s.reuse_stats()["carried_nodes"] >= 129 * (H.REUSE_PLIES - 1)


# ------------------------------------------------------------------ 4. FEN cache
@pytest.mark.parametrize("cap", [64, 1 << 16])
@pytest.mark.parametrize("name", ["hashed", "nanmix64"])
def test_fen_cache_changes_rows_only(require_gpu, name, cap):
    """The same roots searched twice on one handle: the second search finds its rows in the cache -- all of
    them at 65536 entries, what survived eviction at 64 (of the hashed chains' 560 rows nothing does: that
    case is the replacement branch alone).  Both equal the uncached reference, so cached one-hot, NaN and
    +inf priors and NaN values come back bit for bit; rows + hits = the uncached rows."""
    family, sims, roots = H.STEP_CASES[name]
    refs = H.step_refs(name, False)
    s, outs = run_search(family, sims, roots, False, runs=2, cache_capacity=cap)
    for out in outs:
        assert_matches(out, [r.out for r in refs])
    st = check_counters(s, refs, runs=2)
    print("%s, %d entries: rows %d, cache hits %d" % (name, cap, st["evals"], st["cache_hits"]))
    if cap == 1 << 16:
        assert st["cache_hits"] >= sum(r.evals for r in refs)          # the whole second search
    elif name == "nanmix64":
        assert st["cache_hits"] > 0


# ------------------------------------------------------------------ 5. self-play
SP = dict(games=4, sims=16, seed=5, continuous=True, cache_capacity=0)
SP_MOVES = 40


def play(sp, moves):
    """`moves` step()s -> ({game id: its drained EpisodeSteps}, {game id: the moves of a game still in flight})"""
    sp.reset()
    done = {}
    for _ in range(moves):
        sp.step()
        for st in sp.drain():
            done.setdefault(st.game_id, []).append(st)
    return done, {gid: list(mv) for _, gid, _, active, mv in sp.inflight() if active}


@pytest.mark.parametrize("family", ["hashed", "zeros", "uniform", "last"])
def test_selfplay_fresh_trees(require_gpu, family):
    """40 moves of 4 continuous slots; the C oracle replays the handle's eval log (eval_kind = 2), capped at
    the same 40 plies.  Games 0..3 that ended (under `last` all four) are compared ply for ply: visits, action, depth, result, final value.  Of a game still in flight the driver hands
    out its moves only: they equal the oracle's actions -- the weighted sampling when one move holds every
    visit (hashed), the last maximum under exact visit ties (zeros, uniform)."""
    sp = A.SelfPlay(None, evaluator=S.gpu_evaluator(family), record_evals=True, eval_log_cap=1 << 13, **SP)
    done, flying = play(sp, SP_MOVES)
    assert sp.search.stats()["overflow"] == 0
    ref, _, _ = O.selfplay(O.make_cfg(sims=SP["sims"], noise=True, seed=SP["seed"], eval_kind=2), SP["games"],
                           max_plies=SP_MOVES, replay=O.Replay(*sp.search.eval_log()))
    by_game = {}
    for rec in ref:
        by_game.setdefault(rec["game"], []).append(rec)
    first = range(SP["games"])                                  # the games the slots began with
    ended = [g for g in first if g in done]
    assert ended == [g for g in first if by_game[g][0]["result"] != -2]     # the games the oracle ends, no other
    assert sorted(ended + [g for g in first if g in flying]) == list(first)
    compare_steps([st for g in ended for st in done[g]], [rec for g in ended for rec in by_game[g]])
    for g in first:
        if g in flying:
            recs = sorted(by_game[g], key=lambda r: r["ply"])
            assert len(recs) == SP_MOVES and recs[0]["result"] == -2, g
            assert flying[g] == [r["action"] for r in recs], g
    print("%s: games ended %s, in flight %s" % (family, ended, sorted(g for g in flying if g in first)))
    if family == "last":
        assert ended == list(first)                             # whole records were compared, final values included


@pytest.mark.parametrize("family", ["hashed", "zeros", "uniform"])
def test_selfplay_tree_reuse(require_gpu, family):
    """the same 40 moves with tree reuse against the restatement's games 0..3 (test_sharpcases.
    reuse_selfplay_ref): every ply of a game that ended, the moves of one still in flight"""
    sp = A.SelfPlay(None, evaluator=S.gpu_evaluator(family), tree_reuse=True, **SP)
    done, flying = play(sp, SP_MOVES)
    assert sp.search.stats()["overflow"] == 0
    for g in range(SP["games"]):
        ref = H.reuse_selfplay_ref(family, g, SP["seed"], SP["sims"], SP_MOVES)
        if g in flying:
            assert len(ref) == SP_MOVES and ref[-1]["result"] == 0, g
            assert flying[g] == [rec["action"] for rec in ref], g
            continue
        steps = done[g]
        assert [st.ply for st in steps] == list(range(len(ref))) and ref[-1]["result"] != 0, g
        for st, rec in zip(steps, ref):
            assert st.visits == {int(i): int(rec["visits"][i]) for i in np.nonzero(rec["visits"])[0]}, (g, st.ply)
            assert (st.action, st.search_depth, st.result) == (rec["action"], rec["depth"], ref[-1]["result"]), (g, st.ply)
    assert sp.reuse_stats()["carried_visits"] > 0


# ------------------------------------------------------------------ 7. in-engine net, persistent kernel
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("blocks,filters", [(2, 32), (6, 64)])
def test_peaked_net_persistent_kernel(require_gpu, monkeypatch, blocks, filters, dtype):
    """gamma5+peaked weights (policy logits x 64, value pre-activation x 32: the sharpest evaluations the
    in-engine nets are tested on, depth 9 to 10 at 200 simulations): AZ_PERSIST=1 (k_sims32w at 64 filters;
    32 filters have no persistent kernel, both runs then take k_step) against AZ_PERSIST=0, bit-equal; the
    latter's eval log replays bit-exact through the C oracle."""
    w = N.family_weights("gamma5+peaked", A.random_weights(blocks, filters, seed=42), blocks, filters)
    net = A.AlphaZero(blocks, filters, weights=w, dtype=dtype)
    hs = [[], [588], list(H.shuffle_history())]
    sims, runs = 200, {}
    for persist in ("1", "0"):
        monkeypatch.setenv("AZ_PERSIST", persist)
        s = A.BatchedSearch(net, games=len(hs), sims=sims, noise=True, seed=SEED, cache_capacity=0, record_evals=True,
                            eval_log_cap=4096)
        s.set_roots(hs, apply_noise=True)
        assert s.persistent == (persist == "1" and filters >= 64)
        out = s.run()
        st = s.stats()
        assert st["overflow"] == 0 and st["sims"] == sims * len(hs)
        runs[persist] = (out, (st["sims"], st["evals"], st["terminal_leaves"]), s)
    for x, y in zip(runs["1"][0], runs["0"][0]):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    assert runs["1"][1] == runs["0"][1]
    (imp, vis, dep), _, s = runs["0"]
    rep = O.Replay(*s.eval_log())
    cfg = O.make_cfg(sims=sims, noise=True, seed=SEED, eval_kind=2)
    for g, h in enumerate(hs):
        rv, ri, rd, _ = O.search_game(cfg, h, noise=True, noise_key=O.lib().ref_stream_key(SEED, g, len(h), 0), replay=rep)
        assert np.array_equal(vis[g].astype(F), rv) and dep[g] == rd, g
        assert np.array_equal(imp[g].view(np.uint32), ri.view(np.uint32)), g
    print("%dx%d %s: depths %s" % (blocks, filters, dtype, dep.tolist()))
