"""Carrying self-play games across a weight update: az_selfplay_adopt_net / az_search_adopt_net
(SelfPlay.adopt, BatchedSearch.adopt) and az_selfplay_inflight.

The contract: adopting happens between moves; afterwards every active game is in exactly the state
set_roots would produce from that game's history on the updated evaluator (game id, noise ply = its
ply, the same apply_noise), and in continuous mode the start-position template is evaluated again.  So
a game's plies before the adoption are the old net's, bit for bit, every ply from it on equals a fresh
search of that history on the new net, and with an evaluator that did not change the adoption is
invisible.  Bar: BIT-EXACT everywhere."""
import contextlib
import functools
import os

import numpy as np
import pytest

import azchess as A
import test_oracle_search_api as TA
import test_selfplay_schedule as T
from azchess import _lib as L
from test_gpu_search import histories
from test_gpu_selfplay_continuous import check_against, slot_chains

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def env(**kv):
    """environment knobs that az_search_create reads, restored afterwards (usable inside lru_cache)"""
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update(kv)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


# ------------------------------------------------------------------ 1. synthetic evaluator vs the oracle
def adoption_moves():
    """after which moves the run adopts: 1, 137, 138, 400 and the first other move at which a game ends"""
    games, _ = T.oracle_games()
    ended, _, _ = T.schedule({g: len(s) for g, s in games.items()}, T.SLOTS, T.MOVES)
    fixed = {1, 137, 138, 400}
    return fixed | {min(m for m in ended.values() if m not in fixed)}, ended


@pytest.mark.parametrize("variant", ["fused1", "fused0", "cache4"])
def test_adoption_is_invisible_with_an_unchanged_evaluator(require_gpu, monkeypatch, variant):
    """test_gpu_selfplay_continuous.py part (a) -- 8 slots x 560 moves, 16 simulations, synthetic
    evaluator -- with five adoptions in it.  The synthetic evaluator has no generation, so each one
    evaluates the live roots and the template again, draws the noise again and empties the cache; the
    evaluator being the same, every finished game must still equal the oracle's game of its id."""
    if variant in ("fused1", "fused0"):
        monkeypatch.setenv("AZ_FUSED_STEPS", variant[-1])
    adopt_at, want = adoption_moves()
    assert len(adopt_at) == 5 and max(adopt_at) < T.MOVES
    assert any(m in want.values() for m in adopt_at), "no adoption right after a restart"
    sp = A.SelfPlay(None, games=T.SLOTS, sims=T.SIMS, seed=T.SEED, continuous=True,
                    cache_capacity=4 if variant == "cache4" else 0)
    sp.reset()
    games, ended, adopt_rows = {}, {}, 0
    for m in range(1, T.MOVES + 1):
        sp.step()
        for s in sp.drain():
            games.setdefault(s.game_id, []).append(s)
            assert ended.setdefault(s.game_id, m) == m
        if m in adopt_at:
            e0 = sp.search.stats()["evals"]
            sp.adopt()
            adopt_rows += sp.search.stats()["evals"] - e0
    st = sp.search.stats()
    ref_games, _ = T.oracle_games()
    assert set(games) <= set(ref_games)
    check_against(games, ref_games)
    assert ended == want
    lengths = {g: len(s) for g, s in games.items()}
    chains, per_move = slot_chains(ended, lengths, T.SLOTS)
    T.check_conditions(ended, chains, per_move, {g: s[0].result for g, s in games.items()}, lengths)
    assert adopt_rows == 5 * (T.SLOTS + 1)                 # the live roots and the template, each time
    assert st["sims"] == T.SLOTS * T.SIMS * T.MOVES
    assert st["moves"] == T.SLOTS * T.MOVES
    assert st["games_finished"] == len(games)
    assert st["overflow"] == 0


# ------------------------------------------------------------------ 2. network evaluator
SLOTS, SIMS, SEED, BEFORE, AFTER_MAX = 4, 8, 5, 120, 800
CFG = dict(games=SLOTS, sims=SIMS, seed=SEED)


@functools.lru_cache(maxsize=None)
def weights(seed):
    w = A.random_weights(2, 64, seed=seed)
    w.setflags(write=False)
    return w


def new_net(seed):
    return A.AlphaZero(2, 64, weights=weights(seed), dtype="f32")


def make_selfplay(net, persist, cache, noise=True):
    with env(AZ_PERSIST=persist):
        sp = A.SelfPlay(net, continuous=True, cache_capacity=cache, noise=noise, **CFG)
    assert sp.search.persistent == (persist == "1")
    sp.reset()
    return sp


def play(sp, moves, steps, stop=None):
    """up to `moves` moves, every drained EpisodeStep into steps[(game id, ply)]; stops early once
    stop() holds.  Returns the moves played."""
    for m in range(1, moves + 1):
        sp.step()
        for s in sp.drain():
            assert (s.game_id, s.ply) not in steps
            steps[(s.game_id, s.ply)] = s
        if stop is not None and stop():
            return m
    return moves


def finished_ids(steps):
    return {g for g, _ in steps}


@functools.lru_cache(maxsize=None)
def run_x(persist, cache, noise=True):
    """BEFORE moves on net A, update to B, adopt, then on until every game in flight at the adoption
    and one game that started after it have finished.  A game ends within T.MAX_PLIES plies, so
    2 * T.MAX_PLIES <= AFTER_MAX further moves always suffice."""
    net = new_net(42)
    sp = make_selfplay(net, persist, cache, noise)
    steps = {}
    play(sp, BEFORE, steps)
    before = finished_ids(steps)
    net.update(weights(43))
    with pytest.raises(L.AzError, match="weights changed.*az_selfplay_adopt_net"):
        sp.step()
    hits0 = sp.search.stats()["cache_hits"]
    sp.adopt()
    flight = sp.inflight()
    carried = {gid for _, gid, _, _, _ in flight}

    def done():
        fin = finished_ids(steps)
        return carried <= fin and bool(fin - carried - before)
    after = play(sp, AFTER_MAX, steps, done)
    assert done(), "not finished within %d moves of the adoption" % AFTER_MAX
    st = sp.search.stats()
    return dict(steps=steps, flight=flight, before=before, after=after, stats=st, hits_after=st["cache_hits"] - hits0)


@functools.lru_cache(maxsize=None)
def run_y(persist):
    """the same handle on net A with no update: BEFORE moves, inflight(), then on only to bring the
    records of the games in flight out (a game's steps are drained when it ends)"""
    sp = make_selfplay(new_net(42), persist, 0)
    steps = {}
    play(sp, BEFORE, steps)
    flight = sp.inflight()
    carried = {gid for _, gid, _, _, _ in flight}
    play(sp, T.MAX_PLIES, steps, lambda: carried <= finished_ids(steps))
    assert carried <= finished_ids(steps)
    return steps, flight


def adoption_plies(x):
    """{game id: first ply searched after the adoption} of the games in flight at it"""
    return {gid: ply for _, gid, ply, _, _ in x["flight"]}


def is_before(x, gid, ply):
    return gid in x["before"] or ply < adoption_plies(x).get(gid, 0)


def game_actions(steps, gid):
    n = max(p for g, p in steps if g == gid) + 1
    return [steps[(gid, p)].action for p in range(n)]


def record(s):
    return (s.action, s.search_depth, tuple(sorted(s.visits.items())))


def check_fresh_searches_on_b(x, persist, noise, other=None):
    """(ii): every step of run x searched from the adoption on -- the restarted games' ply 0, built from
    the template, included -- has the visits and depth of set_roots(history, game id, noise ply) + run
    on a second handle on net B, 4 histories at a time.  Returns how many of them differ from the step
    of the same (game id, ply) in `other` (a run that did not adopt)."""
    steps, first = x["steps"], adoption_plies(x)
    new = sorted(k for k in steps if not is_before(x, *k))
    started_after = finished_ids(steps) - set(first) - x["before"]
    assert started_after and all((g, 0) in new for g in started_after)
    with env(AZ_PERSIST=persist):
        ref = A.BatchedSearch(new_net(43), noise=noise, cache_capacity=0, **CFG)
    assert ref.persistent == (persist == "1")
    actions = {g: game_actions(steps, g) for g in finished_ids(steps)}
    differs = 0
    for i in range(0, len(new), SLOTS):
        batch = new[i:i + SLOTS]
        batch += [batch[-1]] * (SLOTS - len(batch))
        ref.set_roots([actions[g][:p] for g, p in batch], apply_noise=noise, game_ids=[g for g, _ in batch],
                      noise_plies=[p for _, p in batch])
        _, vis, dep = ref.run()
        for j, k in enumerate(batch):
            want = {int(a): int(vis[j][a]) for a in np.nonzero(vis[j])[0]}
            assert (steps[k].visits, steps[k].search_depth) == (want, int(dep[j])), k
            differs += other is not None and k in other and record(steps[k]) != record(other[k])
    return differs


@pytest.mark.parametrize("persist", ["0", "1"])
def test_net_update_mid_game_equals_fresh_searches(require_gpu, persist):
    """2x64 f32 nets A (seed 42) and B (43), 4 slots, 8 simulations, noise on; through k_step
    (AZ_PERSIST=0) and through the persistent kernel (1).  Run Y plays on past move 120 only so that
    the games in flight there are drained; which of its steps are compared is decided by move 120."""
    x = run_x(persist, 0)
    y_steps, y_flight = run_y(persist)
    steps, flight, first = x["steps"], x["flight"], adoption_plies(x)
    print("AZ_PERSIST=%s: in flight at the adoption %s, %d further moves, finished ids %s"
          % (persist, [(g, p) for _, g, p, _, _ in flight], x["after"], sorted(finished_ids(steps))))
    assert x["after"] <= AFTER_MAX and x["stats"]["overflow"] == 0
    assert all(active for _, _, _, active, _ in flight) and len(first) == SLOTS
    assert any(p > 0 for p in first.values())
    # (iv) inflight() agrees with the drained games' move prefixes, and with run Y's at the same move
    assert sorted(f[1:] for f in flight) == sorted(f[1:] for f in y_flight)
    for _, gid, ply, _, moves in flight:
        assert len(moves) == ply and game_actions(steps, gid)[:ply] == moves, gid
    # (i) before the adoption: the old net's steps, bit for bit those of the uninterrupted run
    old = [k for k in steps if is_before(x, *k)]
    assert len(old) == BEFORE * SLOTS                      # every slot's first 120 moves
    for k in old:
        assert record(steps[k]) == record(y_steps[k]), k
    # (ii) from the adoption on: a fresh search of the history on net B, the restarted games' ply 0 (the
    # template) included
    differs = check_fresh_searches_on_b(x, persist, True, y_steps)
    assert differs > 0, "nets A and B search alike: the test would not see a missed adoption"
    # (iii) every finished game replays legally and ends in the recorded result
    for gid in finished_ids(steps):
        acts = game_actions(steps, gid)
        gs = A.GameState()
        res = [int(A.play_move(gs, a)) for a in acts]
        assert res[:-1] == [L.ONGOING] * (len(acts) - 1), gid
        assert res[-1] == steps[(gid, 0)].result != L.ONGOING, gid
        assert {steps[(gid, p)].result for p in range(len(acts))} == {res[-1]}, gid


def test_restarted_game_is_built_from_the_new_template(require_gpu):
    """The same run with the noise off (k_step path).  With noise on, the 0.25 share of Dirichlet noise
    outweighs these nets' nearly uniform priors (about 1 / 4096 a move), and a restarted game whose root
    was copied from a template still holding net A's priors would search exactly like a fresh one;
    without noise the root's priors alone order its first selections, and A and B rank the start
    position's moves differently."""
    x = run_x("0", 0, False)
    assert x["after"] <= AFTER_MAX and x["stats"]["overflow"] == 0
    check_fresh_searches_on_b(x, "0", False)


# ------------------------------------------------------------------ 3. the stepwise API
def same_roots(a, b, games):
    return all(np.array_equal(x[g].view(np.uint32), y[g].view(np.uint32)) for x, y in zip(a, b) for g in games)


def test_stepwise_adopt_equals_fresh_roots(require_gpu):
    """set_roots / run / advance on net A with one game advanced into a mate (inactive), update to B:
    run refuses; after az_search_adopt_net(noise) it gives the three live games the result of a fresh
    set_roots + run on B, and the inactive game its old visits.

    The random nets' priors are nearly uniform (about 1 / 4096 a move) and their values a few
    hundredths, so at the reference's c_puct the first search would stay on the first move whose value
    it likes; c_puct = 4000 makes the exploration term outweigh every value but a mate's, and with the
    first roots un-noised all 27 moves of the mate-in-one root are tried in turn until the mate is found.
    The roots under test (after advance and after the adoption) are noised."""
    S, seed = 64, 19
    hs = histories(3, 5)
    cfg = dict(games=4, sims=S, seed=seed, noise=True, c_puct=4000.0)
    start = [A.Position.from_fen(TA.MATE_IN_ONE)] + [A.Position.from_fen(TA.START_FEN)] * 3
    net = new_net(42)
    s = A.BatchedSearch(net, **cfg)
    s.set_roots([[]] + hs, apply_noise=False, start=start)
    _, vis, _ = s.run()
    mates = [a for a in np.nonzero(vis[0])[0].tolist() if TA.play_result(TA.MATE_IN_ONE, [], a) == TA.WHITE_WINS]
    assert mates, "no mating move was visited"
    live = [max((a for a in np.nonzero(vis[g + 1])[0].tolist() if TA.play_result(TA.START_FEN, h, a) == L.ONGOING),
                key=lambda a: (vis[g + 1][a], a)) for g, h in enumerate(hs)]
    assert s.advance([mates[0]] + live, apply_noise=True).tolist() == [L.WHITE_WINS] + [L.ONGOING] * 3
    on_a = s.run()
    net.update(weights(43))
    with pytest.raises(L.AzError, match="weights changed.*az_search_adopt_net"):
        s.run()
    evals0 = s.stats()["evals"]
    s.adopt(apply_noise=True)
    assert s.stats()["evals"] - evals0 == 3                # the live roots; no template outside continuous mode
    on_b = s.run()
    ext = [h + [a] for h, a in zip(hs, live)]
    fresh = A.BatchedSearch(new_net(43), **cfg)
    fresh.set_roots([[]] + ext, apply_noise=True, start=start)
    want = fresh.run()
    assert same_roots(on_b, want, (1, 2, 3))
    assert same_roots(on_b, on_a, (0,)) and on_a[1][0].sum() == S
    assert not same_roots(on_b, on_a, (1, 2, 3))           # the two nets do search differently
    s.adopt(apply_noise=True)                              # unchanged generation: nothing happens
    assert same_roots(s.read_roots(), on_b, (0, 1, 2, 3))


# ------------------------------------------------------------------ 4. refusals and no-ops
def roots_and_steps(sp):
    return [record(s) + (s.game_id, s.ply, s.result) for s in sp.drain()], [x.copy() for x in sp.search.read_roots()]


def test_adopt_mid_move_is_refused_and_unchanged_generation_is_a_no_op(require_gpu):
    """Twin handles on one net: what `a` goes through -- an adoption refused after 3 of a move's 8
    simulations, then adoptions with the generation unchanged -- leaves it bit-equal to `b`, which only
    steps; `evals` shows that the no-op adoptions ran no row (and that a real one does)."""
    net = new_net(42)
    a, b = (make_selfplay(net, "0", 0) for _ in range(2))
    for _ in range(3):
        a.step(), b.step()
    assert a.run_sims(3) == (0, -1, False)
    before = a.search.stats()
    with pytest.raises(L.AzError, match="az_selfplay_adopt_net: a move is in progress"):
        a.adopt()
    with pytest.raises(L.AzError, match="az_search_adopt_net: a move is in progress"):
        a.search.adopt(True)
    assert a.search.stats() == before
    assert a.run_sims(SIMS - 3)[2]
    b.step()
    for m in range(40):
        ra, rb = roots_and_steps(a), roots_and_steps(b)
        assert ra[0] == rb[0] and all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(ra[1], rb[1])), m
        if m % 3 == 0:
            e0 = a.search.stats()["evals"]
            a.adopt()                                      # the generation has not moved
            assert a.search.stats()["evals"] == e0
        a.step(), b.step()
    assert a.search.stats() == b.search.stats()
    # an evaluator without a generation always re-evaluates: the live roots and the template are counted
    sy = A.SelfPlay(None, games=SLOTS, sims=SIMS, seed=SEED, continuous=True, cache_capacity=0)
    sy.reset()
    sy.step()
    e0 = sy.search.stats()["evals"]
    sy.adopt()
    assert sy.search.stats()["evals"] - e0 == SLOTS + 1


def test_adopt_with_a_caller_owned_evaluator(require_gpu):
    """AZ_EVAL_CALLBACK has no generation: the caller says that its model changed by calling adopt().
    The evaluator then sees the live roots as one batch and the start position as a batch of its own,
    and the next search equals a fresh handle's on the new model from inflight()'s histories."""
    nets, current, batches = {"A": new_net(42), "B": new_net(43)}, ["A"], []

    def evaluator(states):
        batches.append([s.fen() for s in states])
        return A.process_batch(states, nets[current[0]])

    cfg = dict(games=2, sims=4, seed=SEED, cache_capacity=0)
    sp = A.SelfPlay(None, continuous=True, evaluator=evaluator, **cfg)
    sp.reset()
    for _ in range(3):
        sp.step()
    flight = sp.inflight()
    assert [(ply, len(moves), active) for _, _, ply, active, moves in flight] == [(3, 3, True)] * 2
    current[0], e0 = "B", sp.search.stats()["evals"]
    del batches[:]
    sp.adopt()
    assert [len(b) for b in batches] == [2, 1] and batches[1] == [A.Position.startpos().fen()]
    assert sp.search.stats()["evals"] - e0 == 3
    got = sp.search.run()                                  # the adopted roots, searched in place
    fresh = A.BatchedSearch(None, evaluator=lambda states: A.process_batch(states, nets["B"]), **cfg)
    fresh.set_roots([m for _, _, _, _, m in flight], apply_noise=True, game_ids=[g for _, g, _, _, _ in flight],
                    noise_plies=[p for _, _, p, _, _ in flight])
    assert same_roots(got, fresh.run(), (0, 1))


# ------------------------------------------------------------------ 5. the FEN cache
def test_adopt_empties_the_fen_cache(require_gpu):
    """run X through k_step with a 64-entry FEN cache: the same EpisodeSteps as with the cache off -- an
    entry kept from net A would serve B's search a wrong prior -- and the cache serves hits again after
    the adoption."""
    on, off = run_x("0", 64), run_x("0", 0)
    assert on["steps"].keys() == off["steps"].keys()
    for k, s in on["steps"].items():
        assert record(s) + (s.result,) == record(off["steps"][k]) + (off["steps"][k].result,), k
    assert sorted(f[1:] for f in on["flight"]) == sorted(f[1:] for f in off["flight"])
    print("cache hits after the adoption: %d of %d" % (on["hits_after"], on["stats"]["cache_hits"]))
    assert on["hits_after"] > 0 and off["stats"]["cache_hits"] == 0
