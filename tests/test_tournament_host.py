"""The tournament arena's host side (libaz az_tournament_*), without a device: the pairing order against
ratings.rs's loops, the argument checks that precede the first device call, and the uniforms
evaluate_round_robin tiles over the matches."""
import ctypes as C

import numpy as np
import pytest

from azchess import _lib as L
from azchess import validation as V


def ratings_rs_order(n):
    # ratings.rs:10-11: for i in 0..n { for j in 0..i { evaluate(&players[i], &players[j]) } }
    return [(i, j) for i in range(n) for j in range(i)]


@pytest.mark.parametrize("n", range(2, 17))
def test_matches_and_pairs_follow_the_round_robin_loops(n):
    want = ratings_rs_order(n)
    assert L.lib.az_tournament_matches(n) == n * (n - 1) // 2 == len(want)
    got = []
    for m in range(len(want)):
        i, j = C.c_int(-1), C.c_int(-1)
        assert L.lib.az_tournament_pair(n, m, C.byref(i), C.byref(j)) == 0
        got.append((i.value, j.value))
    assert got == want
    assert V.tournament_matches(n) == want
    for m in (i * (i - 1) // 2 + j for i, j in want):       # the closed form of the header
        assert want[m] == got[m]
    i, j = C.c_int(), C.c_int()
    for bad in (-1, len(want)):
        assert L.lib.az_tournament_pair(n, bad, C.byref(i), C.byref(j)) < 0
        assert "no match" in L.lib.az_last_error().decode()


def test_pool_sizes_outside_the_range_are_refused():
    i, j = C.c_int(), C.c_int()
    for n in (-3, 0, 1, 17, 1000):
        assert L.lib.az_tournament_matches(n) < 0
        assert "2..16" in L.lib.az_last_error().decode()
        assert L.lib.az_tournament_pair(n, 0, C.byref(i), C.byref(j)) < 0
    assert L.lib.az_tournament_pair(4, 0, None, C.byref(j)) < 0
    assert L.lib.az_tournament_pair(4, 0, C.byref(i), None) < 0


def player(kind, net=None, depth=0):
    return L.AzArenaPlayer(kind, net, depth)


def create(players, n=None, games=4, sims=8, cfg=True, out=True):
    recs = (L.AzArenaPlayer * max(len(players), 1))(*players)
    c = L.AzArenaCfg(games, sims, 3, 1.0, 0)
    h = C.c_void_p()
    rc = L.lib.az_tournament_create(recs if players else None, len(players) if n is None else n,
                                    C.byref(c) if cfg else None, 0, C.byref(h) if out else None)
    msg = L.lib.az_last_error().decode()
    assert h.value is None                                   # no handle comes out of a refused call
    return rc, msg


RANDOM = (L.PLAYER_RANDOM,)


@pytest.mark.parametrize("name, args, kw, text", [
    ("null players", [], dict(n=2), "null"),
    ("null cfg", [player(*RANDOM)] * 2, dict(cfg=False), "null"),
    ("null out", [player(*RANDOM)] * 2, dict(out=False), "null"),
    ("one player", [player(*RANDOM)], dict(), "2..16"),
    ("seventeen players", [player(*RANDOM)] * 17, dict(), "2..16"),
    ("negative kind", [player(*RANDOM), player(-1)], dict(), "bad kind of player 1"),
    ("kind past the enum", [player(5), player(*RANDOM)], dict(), "bad kind of player 0"),
    ("external", [player(*RANDOM), player(*RANDOM), player(L.PLAYER_EXTERNAL)], dict(), "player 2 is external"),
    ("base without a net", [player(*RANDOM), player(L.PLAYER_BASE)], dict(), "player 1 is a base-model player without"),
    ("minimax depth 0", [player(L.PLAYER_MINIMAX, None, 0), player(*RANDOM)], dict(), "MiniMax depth of player 0"),
    ("minimax depth 9", [player(*RANDOM), player(L.PLAYER_MINIMAX, None, 9)], dict(), "MiniMax depth of player 1"),
    ("no games", [player(*RANDOM)] * 3, dict(games=0), "games must be positive"),
    ("negative games", [player(*RANDOM)] * 3, dict(games=-2), "games must be positive"),
    ("mcts without sims", [player(*RANDOM), player(L.PLAYER_MCTS)], dict(sims=0), "sims > 0"),
])
def test_create_checks_its_arguments_before_any_device_call(name, args, kw, text):
    rc, msg = create(args, **kw)
    assert rc < 0, name
    assert "az_tournament_create" in msg and text in msg, (name, msg)


def test_null_handles_are_errors():
    live = C.c_int()
    buf = np.zeros(4, np.int32)
    a, b = C.c_double(), C.c_double()
    assert L.lib.az_tournament_reset(None, None, 0) < 0
    assert L.lib.az_tournament_step(None, None, C.byref(live)) < 0
    assert L.lib.az_tournament_results(None, L.i32ptr(buf), L.i32ptr(buf)) < 0
    assert L.lib.az_tournament_live(None, L.i32ptr(buf)) < 0
    assert L.lib.az_tournament_history(None, 0, 0, L.i32ptr(buf), 4) < 0
    assert L.lib.az_tournament_stats(None, C.byref(a), C.byref(b)) < 0
    assert "null" in L.lib.az_last_error().decode()
    assert L.lib.az_tournament_destroy(None) == 0


def test_tiled_uniforms_are_the_pairwise_uniforms_of_every_match():
    seed, G, M = 11, 5, 6
    for ply in (0, 1, 7):
        u = V.tiled_uniforms(seed, G, ply, M)
        assert u.shape == (M, G) and u.dtype == np.float32
        for m in range(M):
            for g in range(G):
                assert u[m, g] == V.choice_uniform(seed, g, ply), (ply, m, g)
        assert np.ascontiguousarray(u).reshape(-1)[3 * G + 2] == V.choice_uniform(seed, 2, ply)   # t = m G + g
    assert (V.tiled_uniforms(seed, G, 0, M) != V.tiled_uniforms(seed, G, 1, M)).any()


def test_elo_rankings_need_the_engine_for_a_tournament():
    with pytest.raises(ValueError):
        V.compute_elo_rankings([V.Player.random(), V.Player.random()], tournament=True)
    with pytest.raises(ValueError):
        V.compute_elo_rankings([V.Player.random(), V.Player.random()], tournament=True, engine=False)
