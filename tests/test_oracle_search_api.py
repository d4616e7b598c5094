"""The conditions the stepwise search API tests (tests/test_gpu_search_api.py) rest on, from the oracle
alone (no GPU):

  * the advance identity: the oracle's traverse_new (tree.rs:239-256) keeps the child's priors, drops
    the grandchildren and zeroes visits and scores, so the search after advancing by action a from
    history h is exactly a fresh search from h + [a] with the noise stream of ply len(h) + 1;
  * the scenario table of az_search_advance: for every row the oracle's own search of the root says
    that the row is what it claims (the action was visited / never visited / is no move, and
    play_move gives the expected result).
"""
import collections
import functools

import numpy as np
import pytest

import oracle as O

ONGOING, DRAW, WHITE_WINS, BLACK_WINS, ILLEGAL = 0, 1, 2, 3, -1     # include/az.h result codes
START_FEN = "rnbqkbnr/pppppppp/8/8/8/8/PPPPPPPP/RNBQKBNR w KQkq - 0 1"

# (dir_alpha, dir_eps, c_puct, temp_moves): the reference's defaults and three settings away from them
SETTINGS = [(0.3, 0.25, 3.0, 15), (1.0, 0.25, 3.0, 0), (2.5, 1.0, 0.5, 1000), (0.03, 0.0, 10.0, 3)]


def stream_key(seed, game, ply):
    return O.lib().ref_stream_key(seed, game, ply, 0)


# ------------------------------------------------------------------ the advance identity
@pytest.mark.parametrize("alpha,eps,c_puct,temp_moves", SETTINGS)
def test_advance_is_a_fresh_search_of_the_extended_history(alpha, eps, c_puct, temp_moves):
    """3 self-play games x their first 12 plies at 16 simulations: the visits and depth the oracle's
    self-play recorded at ply p (a tree re-rooted p times by traverse_new) equal a fresh search of
    the first p actions with the noise stream (seed, game, p, 0)."""
    games, plies, seed = 3, 12, 5
    cfg = O.make_cfg(sims=16, c_puct=c_puct, alpha=alpha, eps=eps, temp_moves=temp_moves, noise=True, seed=seed,
                     eval_kind=0)
    steps, _, _ = O.selfplay(cfg, games, max_plies=plies)
    by_game = collections.defaultdict(list)
    for s in sorted(steps, key=lambda s: (s["game"], s["ply"])):
        by_game[s["game"]].append(s)
    assert sorted(by_game) == list(range(games))
    rerooted = 0
    for g, ss in by_game.items():
        assert [s["ply"] for s in ss] == list(range(len(ss))) and len(ss) <= plies
        actions = [s["action"] for s in ss]
        for p, s in enumerate(ss):
            rv, _, rd, _ = O.search_game(cfg, actions[:p], noise=True, noise_key=stream_key(seed, g, p))
            assert {int(i): float(rv[i]) for i in np.nonzero(rv)[0]} == s["visits"], (g, p)
            assert rd == s["depth"], (g, p)
            rerooted += p > 0
    assert rerooted >= games * 4          # every setting compares re-rooted trees, not only ply 0


# ------------------------------------------------------------------ the scenario table
# One BatchedSearch runs every row at once, so the rows share the simulation count and the seed; a
# row's game id (its noise stream) is its position in the table.  64 simulations is the smallest of
# 16 / 32 / 64 at which the noise-off search visits the mirrored mate of row b (its prior is small);
# the seed is the first at which every row's condition also holds with noise on.
SIMS, SEED = 64, 2


def sq(name):
    return "abcdefgh".index(name[0]) + 8 * (int(name[1]) - 1)


def move_index(pos, frm, to):
    """the move index of the legal move frm -> to (square names) of a RefPos"""
    f, t = sq(frm), sq(to)
    idx = O.legal_indices(pos)
    hits = {int(idx[k]) for k, m in enumerate(O.legal_moves(pos)) if (m[0], m[1]) == (f, t)}
    assert len(hits) == 1, (frm, to, hits)
    return hits.pop()


def game_at(fen, history):
    """the oracle GameState that starts at `fen` with `history` played (every move ongoing)"""
    g = O.Game(O.from_fen(fen))
    for a in history:
        assert g.play_index(a) == ONGOING
    return g


def history_of(fen, moves):
    g, h = O.Game(O.from_fen(fen)), []
    for frm, to in moves:
        a = move_index(g.position, frm, to)
        assert g.play_index(a) == ONGOING
        h.append(a)
    return h


def play_result(fen, history, action):
    return game_at(fen, history).play_index(action)


# pickers: (fen, history, legal indices in `moves` order, oracle visits [4096]) -> action
def named(frm, to):
    return lambda fen, h, legal, vis: move_index(game_at(fen, h).position, frm, to)


def visited_with_result(result):
    """the most visited move that play_move answers with `result`"""
    def pick(fen, h, legal, vis):
        c = [a for a in sorted(set(legal)) if vis[a] > 0 and play_result(fen, h, a) == result]
        return max(c, key=lambda a: (vis[a], a))
    return pick


def most_visited(fen, h, legal, vis):
    return max(sorted(set(legal)), key=lambda a: (vis[a], a))


def least_visited(fen, h, legal, vis):
    return min((a for a in sorted(set(legal)) if vis[a] > 0), key=lambda a: (vis[a], a))


def never_visited(fen, h, legal, vis):
    return min(a for a in set(legal) if vis[a] == 0)


def not_a_move(fen, h, legal, vis):
    return min(set(range(4096)) - set(legal))


def duplicated_index(fen, h, legal, vis):
    dup = sorted(a for a in set(legal) if legal.count(a) == 4)
    return dup[0]


KNIGHTS = [("g1", "f3"), ("g8", "f6"), ("f3", "g1"), ("f6", "g8"), ("g1", "f3"), ("g8", "f6")]
MATE_IN_ONE = "7k/8/6K1/8/8/8/Q7/8 w - - 0 1"

# (row, start FEN, history as (from, to) moves, picker of the action, condition on the oracle's visits,
# expected az_search_advance result)
SPEC = [
    ("a", MATE_IN_ONE, [], named("a2", "a8"), "visited", WHITE_WINS),
    ("b", "8/q7/8/8/8/6k1/8/7K b - - 0 1", [], named("a7", "a1"), "visited", BLACK_WINS),
    ("c", "3k4/8/8/8/8/8/8/3KQ3 b - - 99 150", [], visited_with_result(DRAW), "visited", DRAW),   # 50-move rule
    ("d", "3k4/8/8/8/8/8/8/3KQ3 b - - 0 199", [], visited_with_result(DRAW), "visited", DRAW),     # fullmove 200
    # the knights out and back (tests/test_gpu_rules.py::_valid_histories: its root has occurred twice),
    # one ply further so that a single move can repeat a position the THIRD time: after 7. Ng1 Black's
    # Ng8 is the start position again (start, ply 4, ply 8)
    ("e", START_FEN, KNIGHTS + [("f3", "g1")], named("f6", "g8"), "visited", DRAW),
    ("f", "k7/8/PK6/8/8/8/8/8 w - - 0 1", [], named("a6", "a7"), "visited", DRAW),                 # stalemate
    ("g", MATE_IN_ONE, [], never_visited, "unvisited", ILLEGAL),
    ("h1", START_FEN, [], not_a_move, "no move", ILLEGAL),
    ("h2", START_FEN, [], lambda *a: -1, "no move", ILLEGAL),
    ("h3", START_FEN, [], lambda *a: 4096, "no move", ILLEGAL),
    # a rook / king shuffle at a 90-move clock: the root has occurred before, the clock is near its end
    ("i", "4k3/8/8/8/8/8/8/R3K2R w - - 90 120", [("h1", "h2"), ("e8", "d8"), ("h2", "h1"), ("d8", "e8")],
     most_visited, "visited", ONGOING),
    ("j", START_FEN, KNIGHTS, least_visited, "visited", ONGOING),
    ("k", "4k3/1P6/8/8/8/8/6p1/4K3 w - - 0 1", [], duplicated_index, "visited", ONGOING),          # promotion x 4
    ("l", "4k3/8/8/8/8/8/7P/4K2R w K - 0 1", [], None, "visited", ONGOING),                         # O-O
    ("m", "8/8/8/2k5/3Pp3/8/8/4K3 b - d3 0 1", [], named("e4", "d3"), "visited", ONGOING),          # en passant
    ("n", "k7/8/8/8/8/8/1p6/K7 w - - 0 1", [], named("a1", "b2"), "visited", DRAW),                 # K v K is left
]

Row = collections.namedtuple("Row", "name fen history sims seed action expected condition legal visits improved depth")


def castling_index(fen, h, legal, vis):
    """the index of White's O-O: the one legal move after which the king is on g1 and the rook on f1"""
    pos = game_at(fen, h).position
    idx = O.legal_indices(pos)
    hits = set()
    for k, m in enumerate(O.legal_moves(pos)):
        rank1 = O.to_fen(O.play_unchecked(pos, m)).split()[0].split("/")[-1]
        if rank1 == "5RK1":                      # king g1, rook f1
            hits.add(int(idx[k]))
    assert len(hits) == 1, hits
    return hits.pop()


def search_cfg(noise):
    return O.make_cfg(sims=SIMS, noise=noise, seed=SEED, eval_kind=0)


@functools.lru_cache(maxsize=None)
def scenario_rows(noise):
    """The table for noise on / off (the oracle's visits, and so the picked actions, differ): each Row
    carries the oracle's search of its root, which is also what the GPU's first run must return."""
    rows = []
    for g, (name, fen, moves, pick, condition, expected) in enumerate(SPEC):
        h = history_of(fen, moves)
        legal = [int(i) for i in O.legal_indices(game_at(fen, h).position)]
        vis, imp, dep, _ = O.search_game(search_cfg(noise), h, noise=noise, noise_key=stream_key(SEED, g, len(h)),
                                         start=O.from_fen(fen))
        action = (pick or castling_index)(fen, h, legal, vis)
        rows.append(Row(name, fen, h, SIMS, SEED, int(action), expected, condition, legal, vis, imp, dep))
    return rows


@pytest.mark.parametrize("noise", [False, True])
def test_every_scenario_row_is_what_it_claims(noise):
    rows = scenario_rows(noise)
    assert [r.name for r in rows] == [s[0] for s in SPEC]
    for r in rows:
        assert r.visits.sum() == r.sims
        if r.condition == "visited":
            assert r.action in r.legal and r.visits[r.action] > 0, r.name
            assert play_result(r.fen, r.history, r.action) == r.expected, r.name
        elif r.condition == "unvisited":         # legal, but the search never expanded it
            assert r.action in r.legal and r.visits[r.action] == 0, r.name
            assert play_result(r.fen, r.history, r.action) != ILLEGAL and r.expected == ILLEGAL, r.name
        else:
            assert r.action not in r.legal and r.expected == ILLEGAL, r.name
            if 0 <= r.action < 4096:
                assert play_result(r.fen, r.history, r.action) == ILLEGAL, r.name
    by = {r.name: r for r in rows}
    # the rows are the cases they are named for
    assert by["i"].visits[by["i"].action] == by["i"].visits.max()
    nz = by["j"].visits[by["j"].visits > 0]
    assert by["j"].visits[by["j"].action] == nz.min() and nz.min() < nz.max()     # not the most visited child
    assert by["k"].legal.count(by["k"].action) == 4
    # g: the mate-in-one root has 27 legal moves and most have no expanded child after the search
    assert len(set(by["g"].legal)) == 27 and int((by["g"].visits[sorted(set(by["g"].legal))] == 0).sum()) >= 10
    assert by["h2"].action == -1 and by["h3"].action == 4096 and 0 <= by["h1"].action < 4096
    # m is the en-passant capture: the captured pawn leaves d4
    g = game_at(by["m"].fen, by["m"].history)
    assert g.play_index(by["m"].action) == ONGOING and O.to_fen(g.position).split()[0] == "8/8/8/2k5/8/3p4/8/4K3"
    # e repeats the start position a third time; its history begins with the knights tour of the rules tests
    from test_gpu_rules import _valid_histories
    assert by["e"].history[:6] == [h for f, h in _valid_histories() if f == START_FEN and len(h) == 6][0]
    assert by["j"].history == by["e"].history[:6]
