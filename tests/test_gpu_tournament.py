"""The tournament arena (libaz az_tournament_*: every pairing of a pool of players in one device handle, all
matches advancing in lockstep) on the GPU.  Its reference is the pairwise engine arena, which the existing
tests pin to the host loop and the oracle: every game of every match must come out move for move as
evaluate(players[i], players[j], engine=True) / Arena(players[i], players[j]) plays it."""
import numpy as np
import pytest

import azchess as A
from azchess import _lib as L
from azchess import validation as V

pytestmark = pytest.mark.gpu

MATE_IN_ONE = "6k1/5ppp/8/8/8/8/8/R3K3 w - - 0 1"          # Ra8#
STALEMATING = "7k/5K2/8/8/8/8/8/6Q1 w - - 0 1"             # Qg6 stalemates
KRK_99 = "4k3/8/8/8/8/8/8/R3K3 w - - 99 80"
KRK_98 = "4k3/8/8/8/8/8/8/R3K3 w - - 98 80"
KRK_B199 = "4k3/8/8/8/8/8/8/R3K3 b - - 10 199"
KRK_B198 = "4k3/8/8/8/8/8/8/R3K3 b - - 10 198"


@pytest.fixture(scope="module")
def nets():
    return tuple(A.AlphaZero(2, 32, dtype="f32", seed=s) for s in (4, 5, 6))


def tour_snapshot(tour):
    res, plies = tour.results()
    M, G = len(tour.matches), tour.games
    return (res.tolist(), plies.tolist(), tour.live().tolist(),
            [[tour.history(m, g) for g in range(G)] for m in range(M)], tour.stats())


def arena_snapshot(arena):
    res, plies = arena.results()
    return res.tolist(), plies.tolist(), arena.live().tolist(), [arena.history(g) for g in range(arena.games)]


def match_of(snap, m):
    return snap[0][m], snap[1][m], snap[2][m], snap[3][m]


# ------------------------------------------------------------------ 1. a pool of six == its fifteen matches
@pytest.mark.parametrize("games", [6, 5])
def test_pool_of_six_equals_its_fifteen_pairwise_matches(require_gpu, nets, games):
    n4, n5, _ = nets
    players = [V.Player.base(n4), V.Player.base(n5), V.Player.mcts(None), V.Player.mcts(n4), V.Player.minimax(1),
               V.Player.random()]
    # num_stochastic_moves 3: plies 0-5 are sampled (WeightedIndex), plies 6-23 take the last maximum
    kw = dict(games=games, sims=8, seed=11, max_plies=24, num_stochastic_moves=3)
    rr = V.evaluate_round_robin(players, record=True, **kw)
    matches = V.tournament_matches(len(players))
    assert len(rr) == len(matches) == 15
    wm = [[0.5] * 6 for _ in range(6)]
    for (i, j), (res, hist, result) in zip(matches, rr):
        pres, phist, presult = V.evaluate(players[i], players[j], engine=True, record=True, **kw)
        assert hist == phist, (i, j)
        assert result == presult, (i, j)
        assert (res.winrate, res.p1_winrate, res.p2_winrate, res.drawrate) == (pres.winrate, pres.p1_winrate,
                                                                               pres.p2_winrate, pres.drawrate)
        assert all(len(h) > 0 for h in hist)
        wm[i][j], wm[j][i] = pres.winrate, 1.0 - pres.winrate
    avg, elos, twm = V.compute_elo_rankings(players, 150.0, engine=True, tournament=True, **kw)
    assert twm == wm                                          # the pairwise engine=True matrix, exactly
    assert elos.tolist() == V.compute_elos(wm, 150.0).tolist()
    assert avg == rr[0][0].avg_batch_size > 0


def test_elo_rankings_through_the_tournament_equal_the_pairwise_ones(require_gpu, nets):
    players = [V.Player.base(nets[0]), V.Player.random(), V.Player.base(nets[1]), V.Player.minimax(1)]
    kw = dict(games=5, seed=3, max_plies=20, num_stochastic_moves=2, engine=True)
    _, pelos, pwm = V.compute_elo_rankings(players, 150.0, **kw)
    _, telos, twm = V.compute_elo_rankings(players, 150.0, tournament=True, **kw)
    assert twm == pwm and telos.tolist() == pelos.tolist()


# ------------------------------------------------------------------ 2. statistics
def test_forwards_are_shared_and_rows_are_not(require_gpu, nets):
    players = [V.Player.base(n) for n in nets]
    G, seed, plies = 4, 7, 12
    tour = V.Tournament(players, games=G, seed=seed, num_stochastic_moves=2)
    for ply in range(plies):
        tour.step(V.tiled_uniforms(seed, G, ply, len(tour.matches)))
    ninf, rows = tour.stats()
    pair_ninf, pair_rows, movers = 0.0, 0.0, set()
    for m, (i, j) in enumerate(tour.matches):
        _, hist, pn, pr = V._evaluate_engine(players[i], players[j], G, 1, 2, seed, 0, plies, True)
        assert hist == [tour.history(m, g) for g in range(G)]
        pair_ninf += pn
        pair_rows += pr
        for g, h in enumerate(hist):
            for ply in range(len(h)):                         # game g was live at this ply; White moves on the even ones
                movers.add((ply, i if (g % 2 == 0) == (ply % 2 == 0) else j))
    assert rows == pair_rows > 0
    assert ninf == len(movers)
    assert ninf < pair_ninf
    assert rows / ninf > pair_rows / pair_ninf


# ------------------------------------------------------------------ 3. the engine's own stream
def test_own_stream_equals_pairwise_arenas_with_the_same_seed(require_gpu, nets):
    players = [V.Player.base(nets[0]), V.Player.base(nets[1]), V.Player.random()]
    G, plies = 4, 16

    def play(seed, arenas):
        tour = V.Tournament(players, games=G, seed=seed)
        for ply in range(plies):
            live = tour.step()
            snap = tour_snapshot(tour)
            lives = 0
            for m, arena in enumerate(arenas):
                lives += arena.step()
                assert match_of(snap, m) == arena_snapshot(arena), (ply, m)
            assert live == lives == int(np.sum(snap[2]))
        return snap

    first = play(21, [V.Arena(players[i], players[j], games=G, seed=21) for i, j in V.tournament_matches(3)])
    assert first[1] == [[plies] * G] * 3 or any(r != L.ONGOING for m in first[0] for r in m)
    tour = V.Tournament(players, games=G, seed=22)
    for _ in range(plies):
        tour.step()
    assert tour_snapshot(tour)[3] != first[3]                 # a second seed: other games
    tour.reset(seed=21)
    for _ in range(plies):
        tour.step()
    assert tour_snapshot(tour)[:4] == first[:4]


# ------------------------------------------------------------------ 4. games ending at different plies
def test_games_end_at_different_plies_and_stay_finished(require_gpu, nets):
    fens = [MATE_IN_ONE, STALEMATING, KRK_99, KRK_98, KRK_B199, KRK_B198]
    start = [A.Position.from_fen(f) for f in fens]
    players = [V.Player.base(nets[0]), V.Player.minimax(1), V.Player.random()]
    G, seed = len(fens), 5
    tour = V.Tournament(players, games=G, seed=seed, num_stochastic_moves=1)
    arenas = [V.Arena(players[i], players[j], games=G, seed=seed, num_stochastic_moves=1) for i, j in tour.matches]
    tour.step(V.tiled_uniforms(seed, G, 0, 3))                # a ply from the start position first: reset clears it
    tour.reset(start=start, seed=seed)
    for arena in arenas:
        arena.reset(start=start, seed=seed)
    assert tour_snapshot(tour)[:4] == ([[L.ONGOING] * G] * 3, [[0] * G] * 3, [[True] * G] * 3, [[[]] * G] * 3)
    ended = {}
    for ply in range(5):
        u = V.tiled_uniforms(seed, G, ply, 3)
        before = tour_snapshot(tour)
        live = tour.step(u)
        snap = tour_snapshot(tour)
        for m, arena in enumerate(arenas):
            arena.step(u[m])
            assert match_of(snap, m) == arena_snapshot(arena), (ply, m)
        assert live == int(np.sum(snap[2]))
        for m in range(3):
            for g in range(G):
                if before[0][m][g] != L.ONGOING:              # a finished game stays as it ended
                    assert (snap[0][m][g], snap[1][m][g], snap[3][m][g]) == (before[0][m][g], before[1][m][g],
                                                                           before[3][m][g])
                    assert not snap[2][m][g]
                elif snap[0][m][g] != L.ONGOING:
                    ended[(m, g)] = ply + 1
    # the move limits alone end games 2, 3, 4 and 5 of every match after 1, 2, 1 and 3 plies
    for m in range(3):
        assert [ended[(m, g)] for g in (2, 3, 4, 5)] == [1, 2, 1, 3]
        assert [snap[0][m][g] for g in (2, 3, 4, 5)] == [L.DRAW] * 4


def test_start_positions_an_mcts_search_cannot_hold_are_refused(require_gpu, nets):
    white, black = A.Position.startpos(), A.Position.startpos().play(A.move_to_index(12, 28, 0))
    lopsided = [white, black, white, black]                   # player 1 of every match to move in all four games
    pool = [V.Player.base(nets[0]), V.Player.random(), V.Player.mcts(None)]
    tour = V.Tournament(pool, games=4, sims=8, seed=2)
    assert tour.step(V.tiled_uniforms(2, 4, 0, 3)) == 12
    before = tour_snapshot(tour)
    with pytest.raises(L.AzError, match="MCTS"):
        tour.reset(start=lopsided)
    assert tour_snapshot(tour) == before                      # a refused reset changes nothing
    tour.reset(start=[white, white, black, black])            # two games each: fine
    assert tour.step(V.tiled_uniforms(2, 4, 0, 3)) == 12
    no_mcts = V.Tournament(pool[:2] + [V.Player.minimax(1)], games=4, seed=2)
    no_mcts.reset(start=lopsided)                             # without a search nothing limits the set
    assert no_mcts.step(V.tiled_uniforms(2, 4, 0, 3)) == 12


# ------------------------------------------------------------------ 5. all or nothing
def test_a_non_finite_policy_refuses_the_ply_of_every_match(require_gpu, nets):
    from azchess.agent import param_shapes
    w = A.random_weights(2, 32, seed=4)
    off = 0
    for name, shape, _ in param_shapes(2, 32):
        n = int(np.prod(shape))
        if name == "policy_conv_2.bias":
            w[off:off + n] = np.nan                             # every policy row is NaN
        off += n
    bad = A.AlphaZero(2, 32, weights=w, dtype="f32")
    assert np.isnan(bad.forward(A.to_tensor(A.Position.startpos()))[0]).all()
    # matches (1, 0), (2, 0), (2, 1): the NaN net is player 2 of matches 0 and 1 and has no part in match 2.
    # From these start positions player 1 of every match moves in both games on the even plies
    white, black = A.Position.startpos(), A.Position.startpos().play(A.move_to_index(12, 28, 0))
    tour = V.Tournament([V.Player.base(bad), V.Player.base(nets[1]), V.Player.random()], games=2, seed=9)
    tour.reset(start=[white, black], seed=9)
    assert tour.step(V.tiled_uniforms(9, 2, 0, 3)) == 6
    before = tour_snapshot(tour)
    assert before[1] == [[1, 1]] * 3 and before[4] == (1.0, 2.0)
    for u in (V.tiled_uniforms(9, 2, 1, 3), None):
        with pytest.raises(L.AzError, match=r"match 0 game 0.*non-finite"):
            tour.step(u)
        assert tour_snapshot(tour) == before
