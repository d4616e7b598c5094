"""An MCTS player's own search settings (az_player_search, az_arena_create_with, az_tournament_create_with),
without a device: the symbols, the record's size, and every refusal -- made before the first device call, in a
message that names the player and the field, with no handle returned -- and Player.mcts carrying its settings."""
import ctypes as C
import math

import pytest

from azchess import _lib as L
from azchess.validation import Player

MCTS, BASE, MINIMAX, RANDOM = L.PLAYER_MCTS, L.PLAYER_BASE, L.PLAYER_MINIMAX, L.PLAYER_RANDOM
UNTOUCHED = 0x5A5A5A5A                                        # *out before the call: it must still be there after it


def player(kind, depth=0):
    return L.AzArenaPlayer(kind, None, depth)


def search(sims=0, leaves=0, c_puct=0.0, reserved=0):
    return L.AzPlayerSearch(sims, leaves, c_puct, reserved)


def ref(x):
    return C.byref(x) if x is not None else None


def arena_with(p1, p2, s1, s2, sims=8, games=4):
    cfg = L.AzArenaCfg(games, sims, 3, 1.0, 0)
    h = C.c_void_p(UNTOUCHED)
    rc = L.lib.az_arena_create_with(ref(p1), ref(p2), ref(s1), ref(s2), C.byref(cfg), 0, C.byref(h))
    assert h.value == UNTOUCHED
    return rc, L.lib.az_last_error().decode()


def tournament_with(players, settings, sims=8, games=4):
    recs = (L.AzArenaPlayer * len(players))(*players)
    ss = (L.AzPlayerSearch * len(players))(*settings) if settings is not None else None
    cfg = L.AzArenaCfg(games, sims, 3, 1.0, 0)
    h = C.c_void_p(UNTOUCHED)
    rc = L.lib.az_tournament_create_with(recs, ss, len(players), C.byref(cfg), 0, C.byref(h))
    assert h.value == UNTOUCHED
    return rc, L.lib.az_last_error().decode()


def test_the_symbols_exist_and_the_record_is_16_bytes():
    assert hasattr(L.lib, "az_arena_create_with") and hasattr(L.lib, "az_tournament_create_with")
    assert C.sizeof(L.AzPlayerSearch) == 16
    assert [f[0] for f in L.AzPlayerSearch._fields_] == ["sims", "leaves", "c_puct", "reserved"]


BAD = [
    ("leaves 9", search(leaves=9), MCTS, 8, "leaves"),
    ("leaves -1", search(leaves=-1), MCTS, 8, "leaves"),
    ("sims -1", search(sims=-1), MCTS, 8, "sims"),
    ("c_puct -1", search(c_puct=-1.0), MCTS, 8, "c_puct"),
    ("c_puct inf", search(c_puct=math.inf), MCTS, 8, "c_puct"),
    ("c_puct nan", search(c_puct=math.nan), MCTS, 8, "c_puct"),
    ("reserved 1", search(reserved=1), MCTS, 8, "reserved"),
    ("sims on a random player", search(sims=5), RANDOM, 8, "sims"),
    ("leaves on a random player", search(leaves=2), RANDOM, 8, "leaves"),
    ("c_puct on a minimax player", search(c_puct=1.5), MINIMAX, 8, "c_puct"),
    ("no sims from either side", search(leaves=2), MCTS, 0, "sims"),
]


@pytest.mark.parametrize("name, bad, kind, sims, field", BAD, ids=[b[0] for b in BAD])
def test_the_arena_refuses_a_bad_setting_and_names_player_and_field(name, bad, kind, sims, field):
    good = search(sims=5)
    rc, msg = arena_with(player(MCTS), player(kind, 2), good, bad, sims=sims)
    assert rc < 0 and msg.startswith("az_arena_create_with: "), (name, msg)
    assert "player 2" in msg and field in msg and "player 1" not in msg, (name, msg)
    rc, msg = arena_with(player(kind, 2), player(MCTS), bad, good, sims=sims)
    assert rc < 0 and "player 1" in msg and field in msg and "player 2" not in msg, (name, msg)


@pytest.mark.parametrize("name, bad, kind, sims, field", BAD, ids=[b[0] for b in BAD])
def test_the_tournament_refuses_a_bad_setting_and_names_player_and_field(name, bad, kind, sims, field):
    # a tournament's players count from 0; the bad one is player 2 of [random, mcts, bad]
    rc, msg = tournament_with([player(RANDOM), player(MCTS), player(kind, 2)], [search(), search(sims=5), bad], sims=sims)
    assert rc < 0 and msg.startswith("az_tournament_create_with: "), (name, msg)
    assert "player 2" in msg and field in msg, (name, msg)


def test_one_player_on_both_sides_takes_one_set_of_settings():
    both = player(MCTS)
    rc, msg = arena_with(both, both, search(sims=5, leaves=2), search(sims=5, leaves=4))
    assert rc < 0 and msg.startswith("az_arena_create_with: ") and "player 2" in msg, msg
    rc, msg = arena_with(both, both, None, search(leaves=2))
    assert rc < 0 and "player 2" in msg, msg


def test_without_settings_the_calls_check_what_the_plain_ones_check():
    """NULL settings: the old rules, under the new call's name; cfg->sims = 0 is then still an error."""
    rc, msg = arena_with(player(RANDOM), player(MCTS), None, None, sims=0)
    assert rc < 0 and msg == "az_arena_create_with: an MCTS player needs sims > 0"
    rc, msg = tournament_with([player(RANDOM), player(MCTS)], None, sims=0)
    assert rc < 0 and msg == "az_tournament_create_with: an MCTS player needs sims > 0"
    rc, msg = arena_with(None, player(RANDOM), search(sims=5), None)
    assert rc < 0 and msg == "az_arena_create_with: null player 1"
    rc, msg = tournament_with([player(RANDOM), player(BASE)], [search(), search()])
    assert rc < 0 and msg == "az_tournament_create_with: player 1 is a base-model player without a net"


def test_the_first_bad_player_is_the_one_named():
    rc, msg = tournament_with([player(MCTS), player(MCTS), player(MCTS)],
                              [search(sims=4), search(sims=4, leaves=11), search(sims=-3)])
    assert rc < 0 and "player 1" in msg and "leaves" in msg, msg


def test_player_mcts_carries_its_settings():
    p = Player.mcts(None, sims=5, leaves=4)
    assert (p.kind, p.model, p.sims, p.leaves, p.c_puct) == ("mcts", None, 5, 4, None)
    r = p.search_record()
    assert (r.sims, r.leaves, r.c_puct, r.reserved) == (5, 4, 0.0, 0)
    assert p.search_settings(64, 3.0) == (5, 4, 3.0)
    q = Player.mcts(None)
    assert (q.sims, q.leaves, q.c_puct) == (None, None, None) and q.search_settings(64, 3.0) == (64, 1, 3.0)
    r = Player.random().search_record()
    assert (r.sims, r.leaves, r.c_puct, r.reserved) == (0, 0, 0.0, 0)
