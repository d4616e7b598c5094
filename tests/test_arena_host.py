"""The arena's host side (libaz az_arena_*), without a device: the argument checks of az_arena_create, made
before the first device call and worded as they always were ("player 1" / "player 2"), and the null-handle
errors of every az_arena_* call."""
import ctypes as C

import numpy as np
import pytest

from azchess import _lib as L


def player(kind, net=None, depth=0):
    return L.AzArenaPlayer(kind, net, depth)


def create(p1, p2, games=4, sims=8, cfg=True, out=True):
    c = L.AzArenaCfg(games, sims, 3, 1.0, 0)
    h = C.c_void_p()
    rc = L.lib.az_arena_create(C.byref(p1) if p1 is not None else None, C.byref(p2) if p2 is not None else None,
                               C.byref(c) if cfg else None, 0, C.byref(h) if out else None)
    msg = L.lib.az_last_error().decode()
    assert h.value is None                                   # no handle comes out of a refused call
    return rc, msg


RANDOM = (L.PLAYER_RANDOM,)
BOTH_SIDES = player(L.PLAYER_MCTS)


@pytest.mark.parametrize("name, p1, p2, kw, text", [
    ("null player 1", None, player(*RANDOM), dict(), "az_arena_create: null player 1"),
    ("null player 2", player(*RANDOM), None, dict(), "az_arena_create: null player 2"),
    ("null cfg", player(*RANDOM), player(*RANDOM), dict(cfg=False), "az_arena_create: null argument"),
    ("null out", player(*RANDOM), player(*RANDOM), dict(out=False), "az_arena_create: null argument"),
    ("negative kind", player(-1), player(*RANDOM), dict(), "az_arena_create: bad kind of player 1"),
    ("kind past the enum", player(*RANDOM), player(5), dict(), "az_arena_create: bad kind of player 2"),
    ("base without a net", player(*RANDOM), player(L.PLAYER_BASE), dict(),
     "az_arena_create: player 2 is a base-model player without a net"),
    ("minimax depth 0", player(L.PLAYER_MINIMAX, None, 0), player(*RANDOM), dict(),
     "az_arena_create: MiniMax depth of player 1 outside 1..8"),
    ("minimax depth 9", player(L.PLAYER_EXTERNAL), player(L.PLAYER_MINIMAX, None, 9), dict(),
     "az_arena_create: MiniMax depth of player 2 outside 1..8"),
    ("no games", player(*RANDOM), player(L.PLAYER_EXTERNAL), dict(games=0), "az_arena_create: games must be positive"),
    ("negative games", player(*RANDOM), player(*RANDOM), dict(games=-2), "az_arena_create: games must be positive"),
    ("mcts without sims", player(*RANDOM), player(L.PLAYER_MCTS), dict(sims=0),
     "az_arena_create: an MCTS player needs sims > 0"),
    ("mcts on both sides without sims", BOTH_SIDES, BOTH_SIDES, dict(sims=-1),
     "az_arena_create: an MCTS player needs sims > 0"),
])
def test_create_checks_its_arguments_before_any_device_call(name, p1, p2, kw, text):
    rc, msg = create(p1, p2, **kw)
    assert rc < 0, name
    assert msg == text, (name, msg)


def test_the_first_bad_player_is_the_one_named():
    rc, msg = create(player(L.PLAYER_BASE), player(7))
    assert rc < 0 and msg == "az_arena_create: player 1 is a base-model player without a net"
    both = player(L.PLAYER_MINIMAX, None, 0)                 # one record on both sides is player 1
    rc, msg = create(both, both)
    assert rc < 0 and msg == "az_arena_create: MiniMax depth of player 1 outside 1..8"


@pytest.mark.parametrize("call, args, text", [
    ("reset", lambda b: (None, None, 0), "az_arena_reset: null arena"),
    ("step", lambda b: (None, None, None, C.byref(C.c_int())), "az_arena_step: null arena"),
    ("results", lambda b: (None, L.i32ptr(b), L.i32ptr(b)), "az_arena_results: null arena"),
    ("live", lambda b: (None, L.i32ptr(b)), "az_arena_live: null argument"),
    ("history", lambda b: (None, 0, L.i32ptr(b), 4), "az_arena_history: null arena"),
    ("stats", lambda b: (None, C.byref(C.c_double()), C.byref(C.c_double())), "az_arena_stats: null arena"),
])
def test_null_handles_are_errors(call, args, text):
    buf = np.zeros(4, np.int32)
    assert getattr(L.lib, "az_arena_" + call)(*args(buf)) < 0
    assert L.lib.az_last_error().decode() == text


def test_destroying_no_handle_is_no_error():
    assert L.lib.az_arena_destroy(None) == 0
