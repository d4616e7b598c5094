"""The MCTS players of the match engine (libaz az_arena_create_with / az_tournament_create_with) on the GPU:
every player searches with its own settings (az_player_search), its roots are written by a kernel from the
arena's own position histories (AZ_ARENA_DEVICE_ROOTS), and the searches of one ply run side by side
(AZ_ARENA_OVERLAP).  The references are the host loop of evaluate(engine=False), the pairwise arenas, and the
same engine with the host-side roots and the serial order it had before: every form plays the same moves and
reports the same statistics."""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest

import azchess as A
from azchess import _lib as L
from azchess import validation as V
from azchess.chess import GameState, play_move

pytestmark = pytest.mark.gpu

MCTS = V.Player.mcts


@pytest.fixture(scope="module")
def nets():
    return tuple(A.AlphaZero(2, 32, dtype="f32", seed=s) for s in (4, 5, 6))


@contextlib.contextmanager
def env(**kw):
    """Environment variables the engine reads at create, set around the call and put back."""
    old = {k: os.environ.get(k) for k in kw}
    try:
        for k, v in kw.items():
            os.environ[k] = str(v)
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def arena_snapshot(arena):
    res, plies = arena.results()
    return (res.tolist(), plies.tolist(), arena.live().tolist(), [arena.history(g) for g in range(arena.games)],
            arena.stats())


def tour_snapshot(tour):
    res, plies = tour.results()
    M, G = len(tour.matches), tour.games
    return (res.tolist(), plies.tolist(), tour.live().tolist(),
            [[tour.history(m, g) for g in range(G)] for m in range(M)], tour.stats())


def play_out(handle, start=None, seed=0, max_plies=450, u=None):
    """Reset, then the engine's own stream (or u(ply)) until every game has ended or max_plies."""
    handle.reset(start=start, seed=seed)
    for ply in range(max_plies):
        if handle.step(None if u is None else u(ply)) == 0:
            break
    return handle


# ------------------------------------------------------------------ 1. own settings: engine == host loop
def test_own_settings_engine_equals_host_loop(require_gpu, nets):
    p1, p2 = MCTS(None, sims=12, leaves=4), MCTS(nets[0], sims=5)
    kw = dict(games=5, sims=8, num_stochastic_moves=3, max_plies=16, record=True, seed=13)
    eres, ehist, eresult = V.evaluate(p1, p2, engine=True, **kw)
    hres, hhist, hresult = V.evaluate(p1, p2, engine=False, **kw)
    assert ehist == hhist and eresult == hresult
    assert all(len(h) == 16 for h in ehist) or any(r is not None for r in eresult)
    assert (eres.num_inferences, eres.avg_batch_size) == (hres.num_inferences, hres.avg_batch_size)
    # while all five games are live both players search on every ply: ceil(12 / 4) + 1 = 4 forwards for
    # player 1, 5 + 1 = 6 for player 2 (the match's sims = 8 is nobody's)
    if all(len(h) == 16 for h in ehist):
        assert eres.num_inferences == 16 * 4 + 16 * 6
    assert eres.avg_batch_size > 0


def test_one_leaf_parallel_player_on_both_sides_engine_equals_host_loop(require_gpu, nets):
    both = MCTS(nets[1], leaves=2)                              # G slots; sims from the match
    kw = dict(games=3, sims=9, num_stochastic_moves=2, max_plies=10, record=True, seed=5)
    eres, ehist, eresult = V.evaluate(both, both, engine=True, **kw)
    hres, hhist, hresult = V.evaluate(both, both, engine=False, **kw)
    assert ehist == hhist and eresult == hresult
    assert (eres.num_inferences, eres.avg_batch_size) == (hres.num_inferences, hres.avg_batch_size)
    if all(len(h) == 10 for h in ehist):
        assert eres.num_inferences == 10 * (5 + 1)              # ceil(9 / 2) + 1 per ply


# ------------------------------------------------------------------ 2. zeros change nothing
def raw_arena(players, recs, settings, G, sims, nsm, seed, c_puct=3.0):
    """V.Arena around a handle of az_arena_create (settings is None) or az_arena_create_with."""
    cfg = L.AzArenaCfg(G, sims, nsm, c_puct, seed)
    h = C.c_void_p()
    if settings is None:
        L.check(L.lib.az_arena_create(C.byref(recs[0]), C.byref(recs[1]), C.byref(cfg), 0, C.byref(h)))
    else:
        s1, s2 = (C.byref(s) if s is not None else None for s in settings)
        L.check(L.lib.az_arena_create_with(C.byref(recs[0]), C.byref(recs[1]), s1, s2, C.byref(cfg), 0, C.byref(h)))
    a = V.Arena.__new__(V.Arena)
    a.games, a._players, a._h = G, players, h
    return a


@pytest.mark.parametrize("given_u", [False, True], ids=["own stream", "given uniforms"])
def test_zero_settings_play_the_plain_calls_games(require_gpu, nets, given_u):
    G, sims, nsm, seed, plies = 5, 8, 3, 17, 12
    recs = (L.AzArenaPlayer(L.PLAYER_MCTS, nets[0]._h, 0), L.AzArenaPlayer(L.PLAYER_MCTS, None, 0))
    u = (lambda ply: np.array([V.choice_uniform(seed, g, ply) for g in range(G)], np.float32)) if given_u else None
    snaps = []
    for settings in (None, (None, None), (L.AzPlayerSearch(0, 0, 0.0, 0), None),
                     (L.AzPlayerSearch(0, 0, 0.0, 0), L.AzPlayerSearch(0, 0, 0.0, 0))):
        arena = raw_arena(nets, recs, settings, G, sims, nsm, seed)
        snaps.append(arena_snapshot(play_out(arena, seed=seed, max_plies=plies, u=u)))
    assert all(s == snaps[0] for s in snaps[1:])
    assert all(len(h) > 0 for h in snaps[0][3]) and snaps[0][4][0] > 0
    if all(len(h) == plies for h in snaps[0][3]):
        assert snaps[0][4][0] == 2 * plies * (sims + 1)         # sims + 1 per searching player and ply, as ever


# ------------------------------------------------------------------ 3. a mixed pool == its pairwise arenas
def test_tournament_with_mixed_settings_equals_its_pairwise_arenas(require_gpu, nets):
    a, b, _ = nets
    players = [MCTS(a, sims=8), MCTS(a, sims=8, leaves=4), MCTS(None, sims=16, leaves=8), V.Player.base(b),
               V.Player.random()]
    kw = dict(games=4, sims=6, seed=11, max_plies=12, num_stochastic_moves=3)
    rr = V.evaluate_round_robin(players, record=True, **kw)
    matches = V.tournament_matches(len(players))
    assert len(rr) == len(matches) == 10
    wm = [[0.5] * 5 for _ in range(5)]
    for (i, j), (res, hist, result) in zip(matches, rr):
        pres, phist, presult = V.evaluate(players[i], players[j], engine=True, record=True, **kw)
        assert hist == phist, (i, j)
        assert result == presult, (i, j)
        assert all(len(h) > 0 for h in hist)
        wm[i][j], wm[j][i] = pres.winrate, 1.0 - pres.winrate
    _, elos, twm = V.compute_elo_rankings(players, 150.0, engine=True, tournament=True, **kw)
    assert twm == wm
    assert elos.tolist() == V.compute_elos(wm, 150.0).tolist()
    # the two players on one net differ in `leaves` alone, and that changes their games
    assert rr[matches.index((2, 0))][1] != rr[matches.index((2, 1))][1]


# ------------------------------------------------------------------ 4. device roots == host roots
EN_PASSANT = "rnbqkbnr/1pp1pppp/p7/3pP3/8/8/PPPP1PPP/RNBQKBNR w KQkq d6 0 3"     # exd6 is legal
CASTLING = "r3k2r/pppppppp/8/8/8/8/PPPPPPPP/R3K2R w Kq - 4 10"                  # O-O-O (White), O-O (Black) gone
ENDINGS = ["4k3/8/8/8/8/8/8/R3K3 w - - 90 80", "8/8/3k4/8/8/3K4/8/Q7 w - - 92 90",
           "7k/8/8/8/8/8/R7/K7 w - - 91 70", "8/8/8/4k3/8/8/8/KQ6 w - - 90 100",
           "k7/8/8/8/8/8/8/4K2R w - - 94 60"]
STARTS = [None, EN_PASSANT, CASTLING] + ENDINGS                # all White to move: each side moves in four games


def start_positions():
    return [A.Position.startpos() if f is None else A.Position.from_fen(f) for f in STARTS]


def position_key(p):
    return tuple(p.fen().split()[:4])                           # board, turn, castling, ep: what repeats


def replay(start, moves):
    """The game on the host: (positions after every move, the host's result of the last move or None)."""
    pos, out = start, [start]
    for m in moves:
        pos = pos.play(m)
        out.append(pos)
    result = None
    if start == A.Position.startpos():                         # the host GameState starts there
        g = GameState()
        for m in moves:
            result = int(play_move(g, m))
    return out, result


def roots_cases(nets):
    a, b, c = nets
    return {
        "arena": lambda: V.Arena(MCTS(a, sims=32), MCTS(None, sims=32, leaves=2), games=len(STARTS),
                                 num_stochastic_moves=2, seed=3),
        "arena, one player on both sides": lambda: V.Arena(*(MCTS(b, sims=32),) * 2, games=len(STARTS),
                                                           num_stochastic_moves=2, seed=4),
        "tournament of four": lambda: V.Tournament([MCTS(a, sims=32), MCTS(None, sims=32, leaves=4), V.Player.base(c),
                                                    V.Player.random()], games=len(STARTS), num_stochastic_moves=2,
                                                   seed=5),
    }


_host_roots = {}


@pytest.mark.parametrize("case", ["arena", "arena, one player on both sides", "tournament of four"])
def test_device_roots_equal_host_roots(require_gpu, nets, case):
    make = roots_cases(nets)[case]
    snap = tour_snapshot if case.startswith("tournament") else arena_snapshot
    start = start_positions()
    with env(AZ_ARENA_DEVICE_ROOTS=0):
        host = make()
    with env(AZ_ARENA_DEVICE_ROOTS=1):
        dev = make()
    seed = 29
    hs = snap(play_out(host, start=start, seed=seed))
    ds = snap(play_out(dev, start=start, seed=seed))
    assert ds == hs                                           # moves, results, plies, num_inferences and rows
    assert not np.any(hs[2]), "every game is played to its end"
    _host_roots[case] = hs


def test_the_host_roots_games_ran_into_the_rules_the_roots_carry(require_gpu, nets):
    """From the AZ_ARENA_DEVICE_ROOTS=0 run alone (the engine as it was): at least one game ended by the 50-move
    rule, and at least one game's history holds a position twice -- so repetition counts and the halfmove
    clock were live in the roots the two forms were compared on."""
    if "arena" not in _host_roots:
        test_device_roots_equal_host_roots(require_gpu, nets, "arena")
    res, plies, _, hist, _ = _host_roots["arena"]
    start = start_positions()
    fifty, twice = [], []
    for g, moves in enumerate(hist):
        positions, host_result = replay(start[g], moves)
        assert len(moves) == plies[g]
        if host_result is not None:
            assert host_result == res[g]                      # the host GameState ends the game the same way
        last = positions[-1]
        keys = [position_key(p) for p in positions]
        if len(set(keys)) < len(keys):
            twice.append(g)
        if (res[g] == L.DRAW and last.outcome() == L.ONGOING and last.halfmoves >= 100 and keys.count(keys[-1]) < 3
                and last.fullmoves < 200):
            fifty.append(g)
    print("50-move draws: games %s; a position twice: games %s; plies %s" % (fifty, twice, plies))
    assert fifty, "no game ended by the 50-move rule"
    assert twice, "no game's history holds a position twice"


# ------------------------------------------------------------------ 5. overlap on and off
def test_overlapped_searches_equal_serial_ones(require_gpu, nets):
    a, b, c = nets
    players = [MCTS(a, sims=8, leaves=2), MCTS(b, sims=8), MCTS(c, sims=8, leaves=4), MCTS(b, sims=8, leaves=8)]
    G, seed, plies = 4, 23, 12
    snaps = {}
    for overlap in (0, 1):
        for roots in (0, 1):
            with env(AZ_ARENA_OVERLAP=overlap, AZ_ARENA_DEVICE_ROOTS=roots):
                tour = V.Tournament(players, games=G, sims=8, num_stochastic_moves=3, seed=seed)
            snaps[(overlap, roots)] = tour_snapshot(play_out(tour, seed=seed, max_plies=plies))
    first = snaps[(0, 0)]
    assert all(s == first for s in snaps.values())
    assert all(len(h) > 0 for m in first[3] for h in m) and first[4][1] > 0
    # every player searches on every ply while its games are live: 5, 9, 3 and 2 forwards
    if all(len(h) == plies for m in first[3] for h in m):
        assert first[4][0] == plies * (5 + 9 + 3 + 2)


# ------------------------------------------------------------------ 6. a player with no game to move
def test_a_player_with_no_game_to_move_launches_nothing(require_gpu, nets):
    """Two games, White to move in both: game 0 (player 1 White) ends on its first ply by the 50-move rule,
    and from then on the one live game has one mover per ply -- player 1 (Black in game 1) on the odd plies."""
    p1, p2 = MCTS(nets[0], sims=7, leaves=2), MCTS(None, sims=12)
    arena = V.Arena(p1, p2, games=2, sims=8, num_stochastic_moves=0, seed=1)
    arena.reset(start=[A.Position.from_fen("4k3/8/8/8/8/8/8/R3K3 w - - 99 80"), A.Position.startpos()], seed=1)
    assert arena.step() == 1                                   # both searched: 5 + 13 forwards
    n0, r0 = arena.stats()
    assert n0 == (4 + 1) + (12 + 1) and arena.live().tolist() == [False, True]
    for ply in range(1, 7):
        assert arena.step() == 1
        n1, r1 = arena.stats()
        assert n1 - n0 == ((4 + 1) if ply % 2 == 1 else (12 + 1)), ply      # the mover's forwards alone
        # its one slot: the root row and at most one row per simulation
        assert 1 <= r1 - r0 <= 1 + (7 if ply % 2 == 1 else 12), ply
        n0, r0 = n1, r1
    res, plies = arena.results()
    assert res.tolist() == [L.DRAW, L.ONGOING] and plies.tolist() == [1, 7]
