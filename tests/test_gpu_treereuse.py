"""Tree reuse (az_search_set_tree_reuse, DESIGN.md 5.11: a re-root keeps the played move's subtree, compacted
in place by k_finish, and a move's search tops the root up to `sims` visits) against tests/treereuse_ref.py,
the numpy-f32 restatement of its definition.  Bar: BIT-EXACT visits, improved policies, depths, actions,
results and counters -- through both step forms, every evaluator, the FEN cache, the self-play driver,
chunked moves, weight adoption and train().  The cases' own conditions (the deep case's compactions span
more than one 64-node chunk, the small case carries visits) are asserted in tests/test_treereuse_host.py."""
import functools

import numpy as np
import pytest

import azchess as A
import oracle as O
import treereuse_ref as R
from test_gpu_leafpar import log_evaluator
from test_gpu_search import synthetic_process_batch
from test_treereuse_host import (DEEP_PLIES, DEEP_SIMS, SEED, STEP_PLIES, STEP_SIMS, deep_reference, step_reference,
                                 step_roots)

pytestmark = pytest.mark.gpu
F = np.float32


def last_max(vis_row):
    """training.rs:310-317 on a row of visits: the LAST maximum in index order"""
    idx = np.nonzero(vis_row)[0]
    return int(max(zip(vis_row[idx].tolist(), idx.tolist()))[1])


def drive(s, plies, noise):
    """`plies` plies of run() + advance(last maximum) -> per ply (improved, visits, depth, actions, results)"""
    out = []
    for _ in range(plies):
        imp, vis, dep = s.run()
        actions = [last_max(vis[g]) for g in range(s.games)]
        out.append((imp, vis, dep, actions, s.advance(actions, apply_noise=noise).copy()))
    return out


def assert_stepwise(out, refs):
    """every ply of every game against the restatement; a game that ended is inactive from then on: untouched,
    its read-out the last ply's, its advance result ILLEGAL (-1)"""
    for g, plies in enumerate(refs):
        for p, (imp, vis, dep, actions, res) in enumerate(out):
            rec = plies[min(p, len(plies) - 1)]
            assert np.array_equal(vis[g].astype(F), rec["visits"]), (g, p)
            assert np.array_equal(imp[g].view(np.uint32), rec["improved"].view(np.uint32)), (g, p)
            assert dep[g] == rec["depth"], (g, p)
            assert actions[g] == rec["action"], (g, p)
            assert res[g] == (rec["result"] if p < len(plies) else -1), (g, p)


def totals(refs, plies):
    """the restatement's counters over the first `plies` plies of every game"""
    recs = [rec for game in refs for rec in game[:plies]]
    t = {k: sum(rec[k] for rec in recs) for k in ("sims", "evals", "new_terminal", "known_terminal")}
    kept = [rec for rec in recs if rec["result"] == 0]
    t["reuse"] = dict(reroots=len(kept), carried_visits=sum(rec["next_carried"] for rec in kept),
                      carried_nodes=sum(rec["next_kept"] for rec in kept))
    return t


def assert_counters(s, refs, plies):
    t = totals(refs, plies)
    st = s.stats()
    assert st["overflow"] == 0 and st["max_nodes"] <= st["node_cap"] and st["max_edges"] <= st["edge_cap"], st
    assert st["sims"] == t["sims"], (st, t)
    assert st["evals"] + st["cache_hits"] == t["evals"] and st["terminal_leaves"] == t["new_terminal"], (st, t)
    assert st["sims"] == st["evals"] + st["cache_hits"] + st["terminal_leaves"] + t["known_terminal"], (st, t)
    assert s.reuse_stats() == t["reuse"], (s.reuse_stats(), t["reuse"])
    return st


# ------------------------------------------------------------------ 1. stepwise API
@pytest.mark.parametrize("fused", ["1", "0"])
@pytest.mark.parametrize("noise", [False, True])
def test_stepwise_bit_exact(require_gpu, monkeypatch, noise, fused):
    monkeypatch.setenv("AZ_FUSED_STEPS", fused)
    hs = step_roots()
    s = A.BatchedSearch(None, games=len(hs), sims=STEP_SIMS, noise=noise, seed=SEED, cache_capacity=0, tree_reuse=True)
    assert s.tree_reuse is True and s.persistent is False
    s.set_roots(hs, apply_noise=noise)
    refs = step_reference(noise)
    assert_stepwise(drive(s, STEP_PLIES, noise), refs)
    st = assert_counters(s, refs, STEP_PLIES)
    assert st["cache_hits"] == 0 and s.reuse_stats()["carried_visits"] > 0


# ------------------------------------------------------------------ 2. deep trees
def test_deep_trees_compact_over_several_chunks(require_gpu):
    s = A.BatchedSearch(None, games=1, sims=DEEP_SIMS, noise=False, seed=SEED, cache_capacity=0, tree_reuse=True)
    s.set_roots([[]], apply_noise=False)
    refs = [deep_reference()]
    assert all(rec["next_kept"] >= 65 for rec in refs[0][:3])
    assert_stepwise(drive(s, DEEP_PLIES, False), refs)
    st = assert_counters(s, refs, DEEP_PLIES)
    assert st["overflow"] == 0 and st["max_nodes"] <= st["node_cap"] == DEEP_SIMS + 2


# ------------------------------------------------------------------ 3. self-play driver
SP = dict(games=4, sims=16, seed=5, continuous=True, cache_capacity=0)


@functools.lru_cache(maxsize=None)
def selfplay_reference(game):
    return R.selfplay_game(game, SP["seed"], SP["sims"])


@pytest.mark.parametrize("chunk", [None, 5])
def test_selfplay_records_by_game_id(require_gpu, chunk):
    """4 continuous slots, noise on, default temperature, until two games have finished: their drained
    EpisodeSteps, every ply, equal the restatement's game of the same id -- the sampled and the last-maximum
    move choice, mate and draw markers carried in subtrees, the terminal move.  chunk = 5: the same moves cut
    into az_selfplay_run_sims(5) pieces, each move done when every active root holds `sims` visits."""
    sp = A.SelfPlay(None, tree_reuse=True, **SP)
    assert sp.tree_reuse is True
    sp.reset()
    games, moves = {}, 0
    while len(games) < 2:
        assert moves < 1000, games.keys()                # a game is 400 plies at the most
        if chunk is None:
            sp.step()
        else:
            calls = 1
            while not sp.run_sims(chunk)[2]:
                calls += 1
            assert calls <= -(-SP["sims"] // chunk)
        moves += 1
        for st in sp.drain():
            games.setdefault(st.game_id, []).append(st)
    for gid, steps in games.items():
        ref = selfplay_reference(gid)
        assert [st.ply for st in steps] == list(range(len(ref))), gid
        for st, rec in zip(steps, ref):
            assert st.visits == {int(i): int(rec["visits"][i]) for i in np.nonzero(rec["visits"])[0]}, (gid, st.ply)
            assert (st.action, st.search_depth, st.result) == (rec["action"], rec["depth"], rec["result"]), (gid, st.ply)
            assert F(st.final_value) == rec["final_value"], (gid, st.ply)
    st = sp.search.stats()
    rs = sp.reuse_stats()
    assert st["overflow"] == 0 and st["moves"] == SP["games"] * moves
    # every move but a game's last ends in a re-root that keeps a subtree; what was carried was not run
    # again (the roots now in the slots are re-rooted and not yet searched: their visits are still to be used)
    assert rs["reroots"] == st["moves"] - st["games_finished"]
    waiting = int(sp.search.read_roots()[1].sum())
    assert st["sims"] == st["moves"] * SP["sims"] - (rs["carried_visits"] - waiting) and rs["carried_visits"] > waiting
    assert st["games_finished"] == len(games) >= 2


# ------------------------------------------------------------------ 4. FEN cache
def test_small_fen_cache_changes_rows_only(require_gpu):
    hs = step_roots()
    s = A.BatchedSearch(None, games=len(hs), sims=STEP_SIMS, noise=True, seed=SEED, cache_capacity=64, tree_reuse=True)
    s.set_roots(hs, apply_noise=True)
    refs = step_reference(True)
    assert_stepwise(drive(s, STEP_PLIES, True), refs)
    assert_counters(s, refs, STEP_PLIES)


# ------------------------------------------------------------------ 5. network and callback evaluators
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_network_evaluator(require_gpu, dtype):
    """2x32 net through k_step + the batched tower (reuse never takes the persistent kernel); the restatement
    replays the handle's own evaluations (the eval log)"""
    net = A.AlphaZero(2, 32, weights=A.random_weights(2, 32, seed=42), dtype=dtype)
    hs = step_roots()[:3]
    s = A.BatchedSearch(net, games=3, sims=STEP_SIMS, noise=True, seed=SEED, cache_capacity=0, record_evals=True,
                        eval_log_cap=4096, tree_reuse=True)
    assert s.persistent is False
    s.set_roots(hs, apply_noise=True)
    out = drive(s, 3, True)
    ev = log_evaluator(s)
    refs = [R.stepwise(h, g, 3, STEP_SIMS, SEED, ev) for g, h in enumerate(hs)]
    assert_stepwise(out, refs)
    assert_counters(s, refs, 3)


def test_callback_evaluator(require_gpu):
    hs, calls = step_roots(), []
    s = A.BatchedSearch(None, games=len(hs), sims=STEP_SIMS, noise=True, seed=SEED, cache_capacity=0, tree_reuse=True,
                        evaluator=lambda st: synthetic_process_batch(st, calls))
    s.set_roots(hs, apply_noise=True)
    refs = step_reference(True)
    assert_stepwise(drive(s, STEP_PLIES, True), refs)
    st = assert_counters(s, refs, STEP_PLIES)
    assert calls[0] == len(hs) and sum(calls[1:]) == st["evals"] and max(calls) <= len(hs)


# ------------------------------------------------------------------ 6. adopt() mid-game
def test_adopt_discards_the_carried_subtrees(require_gpu):
    hs = step_roots()
    s = A.BatchedSearch(None, games=len(hs), sims=STEP_SIMS, noise=True, seed=SEED, cache_capacity=0, tree_reuse=True)
    s.set_roots(hs, apply_noise=True)
    refs = step_reference(True)
    out = drive(s, 2, True)
    assert_stepwise(out, refs)
    before, sims0 = s.reuse_stats(), s.stats()["sims"]
    assert before["carried_visits"] > 0
    s.adopt(apply_noise=True)
    assert s.reuse_stats() == before
    imp, vis, dep = s.run()
    live = [g for g in range(len(hs)) if len(refs[g]) > 2]      # the restatement's list ends where the game does
    assert len(live) >= 1
    for g in live:
        moves = list(hs[g]) + [out[p][3][g] for p in range(2)]
        rec = R.Search(moves, O.synth_eval, STEP_SIMS, R.stream_key(SEED, g, len(moves))).run()
        assert rec["carried"] == 0
        assert np.array_equal(vis[g].astype(F), rec["visits"]) and dep[g] == rec["depth"], g
        assert np.array_equal(imp[g].view(np.uint32), rec["improved"].view(np.uint32)), g
    assert s.stats()["sims"] - sims0 == STEP_SIMS * len(live) and s.reuse_stats() == before


# ------------------------------------------------------------------ 7. off is invisible
def test_off_is_invisible(require_gpu):
    hs = step_roots()
    net = A.AlphaZero(6, 64, weights=A.random_weights(6, 64, seed=42), dtype="f32")
    for model in (None, net):
        outs = []
        for touch in (False, True):
            s = A.BatchedSearch(model, games=len(hs), sims=24, noise=True, seed=SEED, cache_capacity=0)
            if touch:
                s.set_tree_reuse(False)
            assert s.tree_reuse is False
            s.set_roots(hs, apply_noise=True)
            outs.append((drive(s, 3, True), s.stats(), s.persistent, s.reuse_stats()))
        for a, b in zip(outs[0][0], outs[1][0]):
            assert all(np.array_equal(x, y) for x, y in zip(a, b))
        assert outs[0][1:] == outs[1][1:]
        assert outs[0][3] == dict(reroots=0, carried_visits=0, carried_nodes=0)
    assert outs[0][2] is True                              # the persistent kernel, as before
    s = A.BatchedSearch(net, games=len(hs), sims=24, seed=SEED, cache_capacity=0, tree_reuse=True)
    assert s.persistent is False and A._lib.lib.az_search_persistent(s._h) == 0


# ------------------------------------------------------------------ 8. refusals
def test_refusals_leave_the_handle_usable(require_gpu):
    hs = step_roots()
    ref = A.BatchedSearch(None, games=len(hs), sims=16, noise=True, seed=SEED, cache_capacity=0)
    ref.set_roots(hs, apply_noise=True)
    want = ref.run()
    s = A.BatchedSearch(None, games=len(hs), sims=16, noise=True, seed=SEED, cache_capacity=0)
    for bad in (2, -1):
        with pytest.raises(A._lib.AzError, match="0 or 1"):
            s.set_tree_reuse(bad)
    assert s.tree_reuse is False
    s.set_roots(hs, apply_noise=True)
    with pytest.raises(A._lib.AzError, match="precede"):
        s.set_tree_reuse(True)
    assert s.tree_reuse is False
    assert all(np.array_equal(x, y) for x, y in zip(s.run(), want))
    sp = A.SelfPlay(None, games=2, sims=4, seed=SEED)
    sp.reset()
    with pytest.raises(A._lib.AzError, match="precede"):
        sp.search.set_tree_reuse(True)
    assert sp.tree_reuse is False and sp.step()[1] == 2
    k = A.BatchedSearch(None, games=len(hs), sims=16, noise=True, seed=SEED, cache_capacity=0, leaves=4)
    with pytest.raises(A._lib.AzError, match=r"tree reuse and leaves > 1"):
        k.set_tree_reuse(True)
    assert k.tree_reuse is False and k.leaves == 4
    k.set_roots(hs, apply_noise=True)
    assert (k.run()[1].sum(axis=1) == 16).all()
    with pytest.raises(A._lib.AzError, match=r"tree reuse and leaves > 1"):
        A.BatchedSearch(None, games=2, sims=4, leaves=2, tree_reuse=True)


# ------------------------------------------------------------------ 9. train(tree_reuse=True)
def test_train_passes_it_to_selfplay(require_gpu, tmp_path):
    args = dict(blocks=2, filters=32, games=4, sims=8, min_replay=1, train_steps=1, batch_size=32, seed=42)
    _, replay, hist = A.train(1, tree_reuse=True, **args)
    assert len(hist) == 1 and hist[0]["selfplay_carried_visits"] > 0
    # the same SelfPlay by hand: train()'s first model and its first pass's seed
    model = A.Trainer(args["blocks"], args["filters"], max_batch=args["batch_size"], seed=args["seed"]).model("f32")
    sp = A.SelfPlay(model, games=args["games"], sims=args["sims"], seed=args["seed"], tree_reuse=True)
    sp.reset()
    mine = A.ReplayBuffer()
    while True:
        _, active = sp.step()
        mine.add_many(sp.drain_raw())
        if active == 0:
            break
    assert hist[0]["selfplay_carried_visits"] == sp.reuse_stats()["carried_visits"]
    assert hist[0]["selfplay_sims"] == sp.search.stats()["sims"] == \
        hist[0]["moves"] * args["sims"] - hist[0]["selfplay_carried_visits"]
    blobs = []
    for name, rp in (("train", replay), ("hand", mine)):
        rp.save(str(tmp_path / name))
        blobs.append((tmp_path / name).read_bytes())
    assert len(mine) == len(replay) > 0 and blobs[0] == blobs[1]
