"""The engine arena (libaz az_arena_*: evaluation games in HBM, one ply per az_arena_step) on the GPU:
its rules against the host rules and the oracle's GameState, its all-or-nothing steps, its matches against
validation.evaluate's host loop (exact equality) and the oracle's replay, its own random stream, and the
Elo step of train()."""
import numpy as np
import pytest

import azchess as A
import oracle as O
from azchess import _lib as L
from azchess import validation as V
from azchess.training import elo_seed, train

pytestmark = pytest.mark.gpu

WHITE_RESULT = {L.DRAW: 0, L.WHITE_WINS: 1, L.BLACK_WINS: -1}


def u_draw(seed, game, ply):
    # the seeded stand-in for thread_rng (an injected input, not part of the rule under test)
    return np.float32(np.random.default_rng([seed, game, ply]).random(dtype=np.float32))


def ext_arena(games):
    return V.Arena(V.Player.external(), V.Player.external(), games=games)


def snapshot(arena):
    res, plies = arena.results()
    return res.tolist(), plies.tolist(), [arena.history(g) for g in range(arena.games)]


# ------------------------------------------------------------------ 1. rules of the ply kernel
def playout_move_lists(seed, ngames):
    parents, actions = O.random_playouts(seed, ngames, 400)
    games = []
    for p, a in zip(parents, actions):
        if p.turn == 0 and p.fullmoves == 1:             # White's first move: a new game
            games.append([])
        games[-1].append(int(a))
    assert len(games) == ngames
    return games


def test_external_games_follow_random_playouts_to_their_ends(require_gpu):
    G = 16
    lists = playout_move_lists(77, G)
    arena = ext_arena(G)
    states = [A.GameState() for _ in range(G)]
    result = [L.ONGOING] * G
    for t in range(max(len(m) for m in lists)):
        actions = np.zeros(G, np.int32)
        for g in range(G):
            if result[g] == L.ONGOING:
                assert t < len(lists[g]), (g, t)
                actions[g] = lists[g][t]
                result[g] = int(A.play_move(states[g], lists[g][t]))
        live = arena.step(actions=actions)
        res, plies, hist = snapshot(arena)
        assert live == sum(r == L.ONGOING for r in result), t
        assert res == result, t
        assert plies == [min(t + 1, len(m)) for m in lists], t
        assert hist == [m[:t + 1] for m in lists], t
    assert live == 0 and all(r != L.ONGOING for r in result)
    assert max(len(m) for m in lists) > 100


MATE_IN_ONE = "6k1/5ppp/8/8/8/8/8/R3K3 w - - 0 1"          # Ra8#
STALEMATING = "7k/5K2/8/8/8/8/8/6Q1 w - - 0 1"             # Qg6 stalemates
KRK_99 = "4k3/8/8/8/8/8/8/R3K3 w - - 99 80"
KRK_98 = "4k3/8/8/8/8/8/8/R3K3 w - - 98 80"
KRK_B199 = "4k3/8/8/8/8/8/8/R3K3 b - - 10 199"
KRK_B198 = "4k3/8/8/8/8/8/8/R3K3 b - - 10 198"
KNIGHTS_OUT = "rnbqkb1r/pppppppp/5n2/8/8/5N2/PPPPPPPP/RNBQKB1R w KQkq - 2 2"


def run_from(arena, fens, lists):
    """reset(start) and play the move lists; every step against the oracle's GameState from the same start."""
    G = arena.games
    arena.reset(start=[A.Position.from_fen(f) for f in fens])
    games = [O.Game(start=O.from_fen(f)) for f in fens]
    result = [L.ONGOING] * G
    t = 0
    while any(r == L.ONGOING and t < len(m) for r, m in zip(result, lists)):
        actions = np.zeros(G, np.int32)
        for g in range(G):
            if result[g] == L.ONGOING:
                actions[g] = lists[g][t]
                result[g] = games[g].play_index(lists[g][t])
                assert result[g] >= 0, (g, t)
        live = arena.step(actions=actions)
        res, plies, hist = snapshot(arena)
        assert res == result, t
        assert live == sum(r == L.ONGOING for r in result)
        assert hist == [m[:p] for m, p in zip(lists, plies)]
        t += 1
    return result, arena.results()[1].tolist()


def test_decisive_moves_and_move_limits_from_start_positions(require_gpu):
    mv = A.move_to_index
    fens = [MATE_IN_ONE, STALEMATING, KRK_99, KRK_98, KRK_B199, KRK_B198]
    lists = [[mv(0, 56, 0)], [mv(6, 46, 0)], [mv(0, 8, 0)], [mv(0, 8, 0)], [mv(60, 52, 1)], [mv(60, 52, 1)]]
    arena = ext_arena(6)
    result, plies = run_from(arena, fens, lists)
    assert result == [L.WHITE_WINS, L.DRAW, L.DRAW, L.ONGOING, L.DRAW, L.ONGOING]
    assert plies == [1] * 6
    # the same handle again: threefold repetition, from the start position and from a start position
    # that is itself one of the three occurrences -- a draw at exactly ply 8 in both
    start = A.Position.startpos().fen()
    out = [mv(6, 21, 0), mv(62, 45, 1), mv(21, 6, 0), mv(45, 62, 1)] * 2
    back = [mv(21, 6, 0), mv(45, 62, 1), mv(6, 21, 0), mv(62, 45, 1)] * 2
    fens = [start, KNIGHTS_OUT] * 3
    result, plies = run_from(arena, fens, [out + [mv(12, 28, 0)], back + [mv(12, 28, 0)]] * 3)
    assert result == [L.DRAW] * 6 and plies == [8] * 6


# ------------------------------------------------------------------ 2. all or nothing
def test_a_refused_step_changes_nothing(require_gpu):
    mv = A.move_to_index
    G = 4
    arena = ext_arena(G)
    e4, d4, e5 = mv(12, 28, 0), mv(11, 27, 0), mv(52, 36, 1)
    own_square = mv(0, 8, 0)                                   # Ra1 onto its own pawn
    before = snapshot(arena)
    for bad_game, bad in ((2, own_square), (1, 5000), (3, -7)):
        actions = np.full(G, e4, np.int32)
        actions[bad_game] = bad
        with pytest.raises(L.AzError, match="game %d" % bad_game):
            arena.step(actions=actions)
        assert snapshot(arena) == before
    with pytest.raises(L.AzError, match="game 0"):
        arena.step()                                            # actions = NULL with external movers
    assert snapshot(arena) == before
    assert arena.step(actions=[e4, d4, e4, d4]) == G
    assert arena.step(actions=[e5] * G) == G
    before = snapshot(arena)
    assert before[1] == [2] * G and before[2][1] == [d4, e5]
    d5 = mv(27, 35, 0)                                          # legal in games 1 and 3 only
    with pytest.raises(L.AzError, match="game 0"):
        arena.step(actions=[d5, d5, mv(6, 21, 0), d5])
    assert snapshot(arena) == before
    assert arena.step(actions=[mv(6, 21, 0), d5, mv(6, 21, 0), d5]) == G
    res, plies, hist = snapshot(arena)
    assert plies == [3] * G and res == [L.ONGOING] * G
    assert hist[1] == [d4, e5, d5] and hist[0] == [e4, e5, mv(6, 21, 0)]


def test_a_non_finite_policy_refuses_the_step(require_gpu):
    from azchess.agent import param_shapes
    w = A.random_weights(2, 32, seed=4)
    off = 0
    for name, shape, _ in param_shapes(2, 32):
        n = int(np.prod(shape))
        if name == "policy_conv_2.bias":
            w[off:off + n] = np.nan                             # every policy row is NaN
        off += n
    net = A.AlphaZero(2, 32, weights=w, dtype="f32")
    assert np.isnan(net.forward(A.to_tensor(A.Position.startpos()))[0]).all()
    G = 4
    arena = V.Arena(V.Player.base(net), V.Player.external(), games=G)   # the net moves first in games 0 and 2
    before = snapshot(arena)
    with pytest.raises(L.AzError, match="game 0.*non-finite"):
        arena.step(u=np.full(G, 0.5, np.float32), actions=np.full(G, A.move_to_index(12, 28, 0), np.int32))
    assert snapshot(arena) == before and arena.stats() == (0.0, 0.0)


# ------------------------------------------------------------------ 3. engine path == host loop
@pytest.fixture(scope="module")
def nets():
    return (A.AlphaZero(2, 32, dtype="f32", seed=4), A.AlphaZero(2, 32, dtype="f32", seed=5))


def pairing(name, nets):
    name = name.replace("_5games", "")
    if name == "mcts_vs_minimax2":
        return V.Player.mcts(None), V.Player.minimax(2)
    if name == "mcts_both_sides":
        p = V.Player.mcts(None)
        return p, p
    if name == "mcts_net_vs_base":
        return V.Player.mcts(nets[0]), V.Player.base(nets[1])
    if name == "base_vs_minimax1":
        return V.Player.base(nets[0]), V.Player.minimax(1)
    if name == "base_vs_base":
        return V.Player.base(nets[0]), V.Player.base(nets[1])
    p = V.Player.base(nets[0])
    return p, p


@pytest.mark.parametrize("name", ["mcts_vs_minimax2", "mcts_both_sides", "base_vs_minimax1", "base_vs_base",
                                  "base_vs_itself", "mcts_net_vs_base", "mcts_vs_minimax2_5games",
                                  "mcts_both_sides_5games"])
def test_engine_match_equals_host_loop(require_gpu, nets, name):
    p1, p2 = pairing(name, nets)
    # 5 games: an MCTS player on one side holds 3 slots and moves in 2 games on the odd plies, so a spare slot
    # repeats its first root
    games = 5 if name.endswith("_5games") else 6
    # num_stochastic_moves 3: plies 0-5 are sampled (WeightedIndex), plies 6-23 take the last maximum
    kw = dict(games=games, sims=8, seed=11, max_plies=24, record=True, num_stochastic_moves=3)
    host, hhist, hres = V.evaluate(p1, p2, engine=False, **kw)
    eng, ehist, eres = V.evaluate(p1, p2, engine=True, **kw)
    assert ehist == hhist
    assert eres == hres
    assert (eng.winrate, eng.p1_winrate, eng.p2_winrate, eng.drawrate) == (host.winrate, host.p1_winrate,
                                                                             host.p2_winrate, host.drawrate)
    assert eng.num_inferences == host.num_inferences
    if name in ("base_vs_base", "base_vs_itself"):
        assert eng.avg_batch_size == host.avg_batch_size


def test_ties_at_the_maximum_take_the_last_legal_index(require_gpu):
    """A net whose policy is uniform (policy_conv_2 zeroed: every logit 0): every legal entry ties at the
    maximum, so past the threshold the mover plays its largest legal index, on the device as on the host."""
    from azchess.agent import param_shapes
    w = A.random_weights(2, 32, seed=6)
    off = 0
    for name, shape, _ in param_shapes(2, 32):
        n = int(np.prod(shape))
        if name.startswith("policy_conv_2."):
            w[off:off + n] = 0.0
        off += n
    net = A.AlphaZero(2, 32, weights=w, dtype="f32")
    pol = net.forward(A.to_tensor(A.Position.startpos()))[0][0]
    assert (pol == pol[0]).all() and pol[0] > 0
    p = V.Player.base(net)
    kw = dict(games=4, seed=13, max_plies=16, record=True, num_stochastic_moves=2)
    host, hhist, hres = V.evaluate(p, p, engine=False, **kw)
    eng, ehist, eres = V.evaluate(p, p, engine=True, **kw)
    assert ehist == hhist and eres == hres and eng == host
    for h in ehist:                                          # replayed on the host rules
        st = A.GameState()
        for ply, a in enumerate(h):
            if st.position.fullmoves > 2:
                assert a == int(st.position.legal_indices().max()), ply
            A.play_move(st, a)


def test_random_mover_counts_under_promotions_four_times(require_gpu):
    """RANDOM: entry min(floor(u n), n - 1) of the legal-move list with its under-promotion duplicates."""
    fen = "8/P6k/8/8/8/8/8/K7 w - - 0 1"                     # a8 promotes: four entries with one index
    legal = [int(a) for a in O.legal_indices(O.from_fen(fen))]
    n = len(legal)
    promo = A.move_to_index(48, 56, 0)
    assert legal.count(promo) == 4 and n == len(set(legal)) + 3
    us = [np.float32((k + 0.5) / n) for k in range(n)]
    us += [np.float32(0.0), np.nextafter(np.float32(1.0), np.float32(0.0)), np.float32(4.0 / n)]
    G = len(us)
    p = V.Player.random()
    arena = V.Arena(p, p, games=G)
    arena.reset(start=[A.Position.from_fen(fen)] * G)
    arena.step(u=np.array(us, np.float32))
    played = [arena.history(g) for g in range(G)]
    want = [[legal[min(int(np.float32(u) * np.float32(n)), n - 1)]] for u in us]
    assert played == want
    assert sum(h == [promo] for h in played[:n]) == 4


def test_mcts_arena_refuses_start_positions_its_search_cannot_hold(require_gpu):
    white, black = A.Position.startpos(), A.Position.startpos().play(A.move_to_index(12, 28, 0))
    arena = V.Arena(V.Player.mcts(None), V.Player.external(), games=4, sims=8)
    e4 = A.move_to_index(12, 28, 0)
    assert arena.step(u=np.zeros(4, np.float32), actions=[e4] * 4) == 4
    before = snapshot(arena)
    with pytest.raises(L.AzError, match="MCTS"):             # player 1 would be to move in all four games
        arena.reset(start=[white, black, white, black])
    assert snapshot(arena) == before                          # a refused reset changes nothing
    arena.reset(start=[white, white, black, black])            # two games each: fine
    assert arena.step(u=np.zeros(4, np.float32), actions=[e4, e4, A.move_to_index(52, 36, 1)] + [0]) == 4


# ------------------------------------------------------------------ 4. oracle replay
def test_engine_mcts_vs_random_replays_through_the_oracle(require_gpu):
    G, sims, seed = 6, 12, 3
    res, hist, result = V.evaluate(V.Player.mcts(None), V.Player.random(), games=G, sims=sims, seed=seed,
                                   max_plies=40, record=True, engine=True)
    cfg = O.make_cfg(sims=sims, noise=False, seed=0, eval_kind=0)
    for g in range(G):
        og = O.Game()
        assert len(hist[g]) == 40 or result[g] is not None
        for ply, a in enumerate(hist[g]):
            u = u_draw(seed, g, ply)
            if (g % 2 == 0) == (ply % 2 == 0):               # the MCTS player is to move
                _, imp, _, _ = O.search_game(cfg, hist[g][:ply], noise=False)
                assert a == O.arena_choose(imp, og.position.fullmoves, 15, u), (g, ply)
            else:
                legal = O.legal_indices(og.position)
                n = len(legal)
                assert a == legal[min(int(np.float32(u) * np.float32(n)), n - 1)], (g, ply)
            r = og.play_index(a)
            assert r >= 0, (g, ply)
            if r != 0:
                assert ply == len(hist[g]) - 1 and result[g] == WHITE_RESULT[r]
            else:
                assert ply < len(hist[g]) - 1 or result[g] is None
    assert abs(res.p1_winrate + res.p2_winrate + res.drawrate - 1.0) < 1e-9


def test_mcts_beside_an_external_seat_replays_through_the_oracle(require_gpu):
    """One step holds MCTS movers, whose improved policy stays on the device for the pick kernel, and an
    external seat's given actions: every MCTS move is the oracle's search under arena_choose, every external
    move the caller's, and the MCTS player accounts sims + 1 inferences per ply in which it moved."""
    G, sims, seed, nsm, plies = 3, 8, 17, 2, 6                # plies 0-3 are sampled, 4-5 take the last maximum
    arena = V.Arena(V.Player.mcts(None), V.Player.external(), games=G, sims=sims, num_stochastic_moves=nsm, seed=seed)
    cfg = O.make_cfg(sims=sims, noise=False, seed=0, eval_kind=0)
    states = [A.GameState() for _ in range(G)]
    hist = [[] for _ in range(G)]
    for ply in range(plies):
        u = np.array([u_draw(seed, g, ply) for g in range(G)], np.float32)
        actions = np.full(G, -1, np.int32)                   # read for the external movers only
        for g in range(G):
            pos = states[g].position
            if (g % 2 == 0) == (ply % 2 == 0):               # the MCTS player is to move
                _, imp, _, _ = O.search_game(cfg, hist[g], noise=False)
                move = O.arena_choose(imp, pos.fullmoves, nsm, u[g])
            else:
                legal = pos.legal_indices()
                move = actions[g] = int(legal[(7 * g + ply) % len(legal)])
            hist[g].append(int(move))
        assert arena.step(u=u, actions=actions) == G
        assert [arena.history(g) for g in range(G)] == hist, ply
        for g in range(G):
            assert int(A.play_move(states[g], hist[g][-1])) == L.ONGOING
    assert arena.stats()[0] == (sims + 1) * plies             # it moved in some game on every ply
    one = V.Arena(V.Player.mcts(None), V.Player.external(), games=1, sims=sims, seed=seed)
    assert one.step() == 1                                    # White: the MCTS player
    assert one.step(actions=[A.move_to_index(52, 36, 1)]) == 1
    assert one.step() == 1
    assert one.stats()[0] == (sims + 1) * 2 and len(one.history(0)) == 3


# ------------------------------------------------------------------ 5. the engine's own stream
def test_engine_stream_is_seeded(require_gpu, nets):
    G, plies = 8, 30

    def play(arena):
        for _ in range(plies):
            if arena.step() == 0:
                break
        return snapshot(arena)

    make = lambda seed: V.Arena(V.Player.base(nets[0]), V.Player.random(), games=G, seed=seed)
    first = make(21)
    m1 = play(first)
    assert m1 == play(make(21))
    assert m1[2] != play(make(22))[2]
    first.reset(seed=22)
    other = play(first)
    assert other[2] != m1[2]
    first.reset(seed=21)
    assert play(first) == m1
    assert first.stats()[0] == plies                          # one forward per ply for the one net


# ------------------------------------------------------------------ 6. train() with the Elo step
def test_train_elo_step_changes_nothing_else(require_gpu):
    ev = A.AlphaZero(2, 32, dtype="f32", seed=9)
    timing = ("selfplay_s", "train_s", "arena_s")
    extra = ("elos", "winrate_matrix", "arena_avg_batch")
    runs = []
    for elo in (None, ev):
        tr, _, hist = train(2, blocks=2, filters=32, games=4, sims=8, min_replay=30, train_steps=2, batch_size=16,
                            seed=5, elo_evaluator=elo, elo_games=4)
        runs.append((tr, hist))
    (tr0, h0), (tr1, h1) = runs
    assert tr0.params().tobytes() == tr1.params().tobytes()
    assert all(k not in h for h in h0 for k in extra + ("arena_s",))
    strip = lambda hist: [{k: v for k, v in h.items() if k not in timing + extra} for h in hist]
    assert strip(h0) == strip(h1)
    for h in h1:
        assert h["elos"][0] == 150.0 and len(h["elos"]) == 2 and h["arena_s"] > 0
    avg, elos, wm = V.compute_elo_rankings([V.Player.base(ev), V.Player.base(tr1.model())], 150.0, games=4,
                                           engine=True, seed=elo_seed(5, 1), device=0)
    assert h1[-1]["elos"] == [float(e) for e in elos]
    assert h1[-1]["winrate_matrix"] == wm
    assert h1[-1]["arena_avg_batch"] == avg
