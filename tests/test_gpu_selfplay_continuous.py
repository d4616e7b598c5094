"""Continuous self-play (a slot whose game ends restarts from the startpos under a new game id:
the tail of k_finish) and the FEN cache under eviction (k_cache_insert's replacement branch and
concurrent-writer skips, the lookup in expand_leaf_wave) against the oracle.  Bar: BIT-EXACT.

The oracle plays games 0..n-1 independently and keys every random stream by (seed, game_id, ply),
so game k of a continuous run must equal oracle game k whichever slot played it: every comparison
here is keyed on game_id, never on the slot.  test_selfplay_schedule.py states, from the oracle
alone, that the configuration of part (a) restarts slots, ends several games in one move and
reaches every result."""
import functools
import os
import time

import numpy as np
import pytest

import azchess as A
import oracle as O
import test_selfplay_schedule as T
from test_gpu_search import compare_steps, histories

pytestmark = pytest.mark.gpu


def play_continuous(sp, moves, k=None):
    """`moves` moves of every slot through step() (k = None) or run_sims(k) chunks, drained after
    every move.  Returns ({game_id: [EpisodeSteps]}, {game_id: move at which it ended, from 1})."""
    games, ended = {}, {}
    for m in range(1, moves + 1):
        if k is None:
            sp.step()
        else:
            while not sp.run_sims(k)[2]:
                pass
        for s in sp.drain():
            games.setdefault(s.game_id, []).append(s)
            assert ended.setdefault(s.game_id, m) == m, "game %d drained at two moves" % s.game_id
    return games, ended


def slot_chains(ended, lengths, slots):
    """The slots' game sequences rebuilt from when each finished game ended and how long it was:
    a game with id >= slots began at the move its predecessor in the slot ended (ids 0..slots-1
    began at move 0).  Games that ended in the same move are interchangeable as predecessors."""
    began = {g: ended[g] - lengths[g] for g in ended}
    per_move = {}
    for g, m in ended.items():
        per_move.setdefault(m, []).append(g)
    chain_of, chains = {}, []
    for g in sorted(ended, key=lambda g: (began[g], g)):
        if g < slots:
            assert began[g] == 0, (g, began[g])
            chain_of[g] = len(chains)
            chains.append([g])
            continue
        # a restart: some finished game of that move has no successor yet
        free = [p for p in per_move.get(began[g], []) if p in chain_of and chains[chain_of[p]][-1] == p]
        assert free, "game %d began at move %d, at which no slot became free" % (g, began[g])
        chain_of[g] = chain_of[free[0]]
        chains[chain_of[g]].append(g)
    return chains, per_move


def check_against(games, ref_games):
    """every finished game == the reference's game of the same id (compare_steps: game_id, ply,
    action, search_depth, result, visits, final_value as f32), no ply missing."""
    for gid, steps in games.items():
        assert sorted(s.ply for s in steps) == list(range(len(steps))), gid
        assert len({s.result for s in steps}) == 1, gid
    compare_steps([s for g in games.values() for s in g], [s for gid in games for s in ref_games[gid]])


# ------------------------------------------------------------------ (a) synthetic evaluator vs the oracle
def run_synthetic(cache=0, k=None):
    sp = A.SelfPlay(None, games=T.SLOTS, sims=T.SIMS, seed=T.SEED, continuous=True, cache_capacity=cache)
    sp.reset()
    games, ended = play_continuous(sp, T.MOVES, k)
    return games, ended, sp.search.stats()


@pytest.mark.parametrize("variant", ["fused1", "fused0", "run_sims5", "cache4"])
def test_continuous_synthetic_matches_oracle_by_game_id(require_gpu, monkeypatch, variant):
    """8 slots x 560 moves, 16 simulations: every finished game equals the oracle's game of its id;
    the finished ids are the ones the schedule predicts; the window's counters add up.  Variants:
    k_step / separate kernels, moves cut into 5-simulation chunks (5 does not divide 16), and a
    4-entry FEN cache (continuous mode and eviction together)."""
    if variant in ("fused1", "fused0"):
        monkeypatch.setenv("AZ_FUSED_STEPS", variant[-1])
    t0 = time.perf_counter()
    games, ended, st = run_synthetic(cache=4 if variant == "cache4" else 0, k=5 if variant == "run_sims5" else None)
    print("%s: %d moves in %.2f s, finished ids %s, cache hits %d"
          % (variant, T.MOVES, time.perf_counter() - t0, sorted(games), st["cache_hits"]))
    ref_games, results = T.oracle_games()
    assert set(games) <= set(ref_games)
    check_against(games, ref_games)
    # the conditions of test_selfplay_schedule on what the GPU produced
    lengths = {g: len(s) for g, s in games.items()}
    chains, per_move = slot_chains(ended, lengths, T.SLOTS)
    T.check_conditions(ended, chains, per_move, {g: s[0].result for g, s in games.items()}, lengths)
    assert max(len(v) for v in per_move.values()) >= 3
    # exactly the ids (and the moves at which they end) the schedule predicts from the oracle
    want, _, _ = T.schedule({g: len(s) for g, s in ref_games.items()}, T.SLOTS, T.MOVES)
    assert ended == want
    assert st["sims"] == T.SLOTS * T.SIMS * T.MOVES
    assert st["moves"] == T.SLOTS * T.MOVES
    assert st["games_finished"] == len(games)
    assert st["overflow"] == 0
    assert st["max_nodes"] <= T.SIMS + 2
    if variant != "cache4":
        assert st["cache_hits"] == 0


# ------------------------------------------------------------------ (b) network evaluator, persistent kernel
NET_GAMES, NET_SIMS, NET_SEED, NET_MOVES = 4, 8, 5, 800


@functools.lru_cache(maxsize=None)
def _net():
    return A.AlphaZero(2, 64, weights=A.random_weights(2, 64, seed=42), dtype="f32")


@functools.lru_cache(maxsize=None)
def run_net_continuous(persist):
    old = os.environ.get("AZ_PERSIST")
    os.environ["AZ_PERSIST"] = persist
    try:
        sp = A.SelfPlay(_net(), games=NET_GAMES, sims=NET_SIMS, seed=NET_SEED, continuous=True, cache_capacity=0)
    finally:
        if old is None:
            del os.environ["AZ_PERSIST"]
        else:
            os.environ["AZ_PERSIST"] = old
    assert sp.search.persistent == (persist == "1")
    sp.reset()
    t0 = time.perf_counter()
    games, ended = play_continuous(sp, NET_MOVES)
    print("AZ_PERSIST=%s: %d moves in %.2f s, finished ids %s" % (persist, NET_MOVES, time.perf_counter() - t0, sorted(games)))
    return games, ended, sp.search.stats()


@functools.lru_cache(maxsize=None)
def run_net_whole_games(n):
    """games 0..n-1 played to the end, not continuous (the path test_selfplay_net_replay_bit_exact
    pins to the oracle); network rows do not depend on the batch they run in."""
    t0 = time.perf_counter()
    _, steps = A.run_all_episodes(_net(), games=n, sims=NET_SIMS, seed=NET_SEED, cache_capacity=0)
    print("%d whole games in %.2f s" % (n, time.perf_counter() - t0))
    ref = {}
    for s in steps:
        ref.setdefault(s.game_id, []).append(
            dict(game=s.game_id, ply=s.ply, action=s.action, depth=s.search_depth, result=s.result,
                 visits=s.visits, final_value=s.final_value))
    assert sorted(ref) == list(range(n))
    return ref


@pytest.mark.parametrize("persist", ["1", "0"])
def test_continuous_net_matches_whole_games_by_game_id(require_gpu, persist):
    """2x64 f32 network, 4 slots x 800 moves, 8 simulations, through k_sims32w (AZ_PERSIST=1) and
    through k_step + the batched tower (0): every finished game equals the same-id game of a
    non-continuous run of ids 0..M-1 with the same network and seed.  A game lasts at most 398
    plies (200-fullmove rule), so in 800 moves every slot finishes at least two games."""
    games, ended, st = run_net_continuous(persist)
    assert len(games) >= 6 and sum(g >= NET_GAMES for g in games) >= 2
    lengths = {g: len(s) for g, s in games.items()}
    assert max(lengths.values()) <= T.MAX_PLIES
    chains, _ = slot_chains(ended, lengths, NET_GAMES)
    assert len(chains) == NET_GAMES and min(len(c) for c in chains) >= 2
    check_against(games, run_net_whole_games(max(games) + 1))
    assert st["sims"] == NET_GAMES * NET_SIMS * NET_MOVES and st["moves"] == NET_GAMES * NET_MOVES
    assert st["games_finished"] == len(games) and st["overflow"] == 0


def test_continuous_net_persistent_equals_step_kernels(require_gpu):
    (g1, e1, s1), (g0, e0, s0) = run_net_continuous("1"), run_net_continuous("0")
    assert e1 == e0
    key = lambda s: (s.game_id, s.ply, s.action, s.search_depth, s.result, np.float32(s.final_value).tobytes(),
                     tuple(sorted(s.visits.items())))
    for gid in g1:
        assert sorted(map(key, g1[gid])) == sorted(map(key, g0[gid])), gid
    assert {k: s1[k] for k in ("sims", "evals", "terminal_leaves", "moves", "games_finished", "overflow")} == \
           {k: s0[k] for k in ("sims", "evals", "terminal_leaves", "moves", "games_finished", "overflow")}


# ------------------------------------------------------------------ (c) FEN cache under eviction, search mode
@functools.lru_cache(maxsize=None)
def _search_reference():
    hs = histories(16, 77)
    cfg = O.make_cfg(sims=200, noise=True, seed=4, eval_kind=0)
    return hs, [O.search_game(cfg, h, noise=True, noise_key=O.lib().ref_stream_key(4, g, len(h), 0))[:3]
                for g, h in enumerate(hs)]


def check_search(out, ref):
    imp, vis, dep = out
    for g, (rv, ri, rd) in enumerate(ref):
        assert np.array_equal(vis[g].astype(np.float32), rv), g
        assert np.array_equal(imp[g].view(np.uint32), ri.view(np.uint32)), g
        assert dep[g] == rd, g


def test_fen_cache_eviction_search_bit_exact(require_gpu):
    """test_fen_cache_search_bit_exact's case (16 games, 200 simulations) with caches of 1, 4, 64
    and 256 entries -- far fewer than the 3200 positions evaluated, so every insert after the first
    few replaces an entry -- next to no cache and one that never fills: visits, improved policy
    and depth equal the oracle's for every capacity; a hit replaces exactly one evaluation.

    The 16 games share no position and a game seldom reaches one twice (26 hits with a cache that
    never fills), and 16 rows are inserted per step, so an entry of a 64-entry table is replaced
    within about 4 steps: measured on the MI355X, capacities 1, 4, 64 and 128 give 0 hits on the
    oracle-equal run; 256, the next power of two that gives any (2; then 512: 4, 1024: 12,
    2048: 21, 4096: 24, 8192 and up: 26), carries the hits > 0 assertion."""
    hs, ref = _search_reference()
    hits, total = {}, {}
    for cap in (0, 1, 4, 64, 256, 1 << 16):
        s = A.BatchedSearch(None, games=len(hs), sims=200, noise=True, seed=4, cache_capacity=cap)
        s.set_roots(hs, apply_noise=True)
        check_search(s.run(), ref)
        st = s.stats()
        hits[cap], total[cap] = st["cache_hits"], st["evals"] + st["cache_hits"]
        assert st["sims"] == len(hs) * 200 and st["overflow"] == 0
    print("cache hits by capacity:", hits, "evals + hits:", total)
    assert len(set(total.values())) == 1, total
    assert hits[0] == 0
    assert hits[1 << 16] >= hits[256] >= hits[64] >= hits[4]
    assert hits[256] > 0


# ------------------------------------------------------------------ (d) many equal rows in one insert launch
def test_fen_cache_equal_rows_in_one_launch(require_gpu):
    """32 games from the startpos: the first simulation steps evaluate the same few positions in
    many games at once, so one k_cache_insert launch holds many rows with one key (and, with 2
    entries, rows racing to replace one slot).  Each game equals the oracle's search with
    game_id = slot, whatever the capacity."""
    G, S, seed = 32, 32, 6
    cfg = O.make_cfg(sims=S, noise=True, seed=seed, eval_kind=0)
    ref = [O.search_game(cfg, [], noise=True, noise_key=O.lib().ref_stream_key(seed, g, 0, 0))[:3] for g in range(G)]
    hits, total = {}, {}
    for cap in (0, 2, 64):
        s = A.BatchedSearch(None, games=G, sims=S, noise=True, seed=seed, cache_capacity=cap)
        s.set_roots([[]] * G, apply_noise=True)
        check_search(s.run(), ref)
        st = s.stats()
        hits[cap], total[cap] = st["cache_hits"], st["evals"] + st["cache_hits"]
        assert st["sims"] == G * S and st["overflow"] == 0
    print("cache hits by capacity:", hits, "evals + hits:", total)
    assert len(set(total.values())) == 1, total
    assert hits[0] == 0
    # the startpos has 20 children, so the 32 leaves of step 0 are at most 20 positions, all of
    # which fit 64 entries: a game whose next simulation opens another root child finds it there
    assert hits[64] > 0
