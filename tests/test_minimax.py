"""The MiniMax(n) arena opponent (chess.rs:248-322) on the host: az_minimax_scores(AZ_DEVICE_HOST)
against a Python restatement over the oracle's rules (tests/minimax_ref.py) -- moves, promotion
roles, scores and negamax call counts, bit for bit -- az_minimax_best's tie rule, get_best_move's
under-promotion quirk (chess.rs:165-167), the arena's MiniMax player and the input checks."""
import ctypes as C

import numpy as np
import pytest

import azchess as A
import oracle as O
from azchess import _lib as L
from azchess import chess as CH
from azchess import validation as V

import minimax_ref as R

HOST = CH.DEVICE_HOST


def position(fen):
    return A.Position.startpos() if fen is None else A.Position.from_fen(fen)


def assert_same(got, nodes, ref, what):
    mv, pr, sc = got
    rmv, rpr, rsc, rcalls = ref
    assert np.array_equal(mv, rmv), what
    assert np.array_equal(pr, rpr), what
    assert np.array_equal(sc, rsc), what
    assert int(nodes) == rcalls, what


@pytest.mark.parametrize("depth", [1, 2, 3])
def test_host_path_equals_reference_on_the_table(depth):
    entries, nodes = CH.minimax_scores([position(f) for _, f in R.TABLE], depth, HOST)
    for i, (name, fen) in enumerate(R.TABLE):
        assert_same(entries[i], nodes[i], R.scores_of_fen(fen, depth), (name, depth))


def host(name, depth):
    (e,), n = CH.minimax_scores([position(R.FENS[name])], depth, HOST)
    return e[0], e[1], e[2], int(n[0])


def test_known_results():
    """the figures the issue records for the table (computed there with such a reference)"""
    mv, pr, sc, n = host("startpos", 3)
    assert len(sc) == 20 and not sc.any() and n == 9322
    for depth, best in ((1, 330), (2, 10), (3, 330)):
        mv, pr, sc, n = host("kiwipete", depth)
        assert len(sc) == 48 and sc.max() == best and (sc == best).sum() == 1
    assert n == 99949
    mv, pr, sc, n = host("pos4", 3)
    assert sc.tolist() == [-300] * 6 and n == 9737
    a1a8 = CH.move_to_index(0, 56, 0)
    for depth in (1, 2, 3):
        mv, pr, sc, n = host("mate_in_1", depth)
        assert sc.max() == 20000 + depth - 1 and (sc == sc.max()).sum() == 1 and mv[sc.argmax()] == a1a8
        if depth == 2:
            assert set(np.delete(sc, sc.argmax()).tolist()) == {500}
    mv, pr, sc, n = host("mate_in_2", 3)
    assert sc.max() == 20002 and (sc == 20002).sum() == 2
    mv, pr, sc, n = host("stalemate_promo", 2)
    assert pr.tolist() == [4, 3, 2, 1, 0, 0, 0, 0, 0]
    assert sc.tolist() == [0, 500, 0, 0, 100, 100, 100, 100, 100]
    mv, pr, sc, n = host("promo_two_mates", 2)
    assert pr.tolist() == [4, 3, 2, 1, 0, 0, 0] and sc.tolist() == [20001, 300, 20001, 120, -100, -100, -100]
    for depth, nodes in ((1, 4), (2, 55), (3, 331)):
        mv, pr, sc, n = host("capture_into_kvk", depth)
        assert sorted(sc.tolist()) == [-500, -500, -500, 0] and n == nodes
        assert mv[sc.argmax()] == CH.move_to_index(19, 28, 0)          # Kd3xe4 leaves K v K: not expanded
    mv, pr, sc, n = host("en_passant", 3)
    assert sc.max() == 100 and (sc == 100).sum() == 4
    mv, pr, sc, n = host("castling", 3)
    assert sc.max() == 1000 and (sc == 1000).sum() == 2 and n == 14338
    mv, pr, sc, n = host("black_promo", 1)
    assert len(sc) == 11 and pr[:4].tolist() == [4, 3, 2, 1] and sc[:4].tolist() == [900, 500, 0, 0]
    assert sc[4:].tolist() == [100] * 7                  # K+B v K and K+N v K are insufficient material: 0


def test_the_issues_black_promotion_fen_is_not_a_position():
    """Its white king stands in check with Black to move (see minimax_ref.ISSUE_BLACK_PROMO_FEN): the
    position check the entry point must run (setup_error) refuses it, so the table holds the same
    ending with the king out of check.  The issue's figures for it (15 entries, best 900 / 100 / 900)
    include captures of the king and are not reproduced."""
    with pytest.raises(L.AzError, match="in check"):
        A.Position.from_fen(R.ISSUE_BLACK_PROMO_FEN)
    assert len(O.legal_moves(O.from_fen(R.ISSUE_BLACK_PROMO_FEN))) == 15


def test_startpos_depth_4_counts_perft():
    (e,), n = CH.minimax_scores([A.Position.startpos()], 4, HOST)
    assert int(n[0]) == 20 + 400 + 8902 + 197281 == 206603
    assert len(e[2]) == 20 and not e[2].any()


def test_playout_positions_depth_2_one_call():
    fens = R.playout_fens()
    assert len(fens) == 48
    entries, nodes = CH.minimax_scores([position(f) for f in fens], 2, HOST)
    for i, fen in enumerate(fens):
        ref = R.scores_of_fen(fen, 2)
        assert len(ref[0]) > 0                                         # none is terminal
        assert_same(entries[i], nodes[i], ref, fen)
    assert int(nodes.sum()) == 57725


def test_minimax_best_tie_rule():
    sc = np.array([5, 9, -3, 9, 9, 0], np.int32)
    ties = [1, 3, 4]
    below_one = np.nextafter(np.float32(1), np.float32(0))
    for u in (0.0, 0.2, 1 / 3, 0.34, 0.5, 0.66, 0.67, 0.99, float(below_one)):
        exp = ties[min(int(np.floor(np.float32(u) * np.float32(3))), 2)]
        assert CH.minimax_best(sc, u) == exp == R.best_entry(sc, u), u
    assert CH.minimax_best(sc, 0.0) == 1 and CH.minimax_best(sc, below_one) == 4
    assert CH.minimax_best(np.array([7], np.int32), 0.9) == 0
    assert L.lib.az_minimax_best(L.i32ptr(sc), 0, C.c_float(0.5)) == -1


def test_get_best_move_plays_the_queen_for_the_rook():
    """the bot prefers f8=R (500; f8=Q stalemates), the arena's move_to_index / index_to_move round
    trip turns that into f8=Q (chess.rs:165-167), and the game is drawn"""
    pos = position(R.FENS["stalemate_promo"])
    (mv, pr, sc), = CH.minimax_scores([pos], 2, HOST)[0]
    k = CH.minimax_best(sc, 0.5)
    assert pr[k] == 3 and sc[k] == 500
    a = CH.get_best_move(pos, 2, 0.5, device=HOST)
    assert a == mv[k] == CH.move_to_index(53, 61, 0)
    assert pos.play(a).outcome() == A.GameResult.Draw
    assert CH.get_best_move(position("7k/5Q2/6K1/8/8/8/8/8 b - - 0 1"), 2, 0.5, device=HOST) is None


def test_arena_minimax_on_the_host_replays_through_the_reference():
    G, seed, depth = 4, 3, 2
    res, hist, result = V.evaluate(V.Player.minimax(depth, device=-1), V.Player.random(), games=G, max_plies=30,
                                   seed=seed, record=True)
    checked = 0
    for g in range(G):
        og = O.Game()
        for ply, a in enumerate(hist[g]):
            if (g % 2 == 0) == (ply % 2 == 0):                         # the MiniMax player is to move
                mv, _, sc, _ = R.scores_of(og.position, depth)
                assert a == mv[R.best_entry(sc, V.choice_uniform(seed, g, ply))], (g, ply)
                checked += 1
            r = og.play_index(a)
            assert r >= 0, (g, ply)
            if r != 0:
                assert ply == len(hist[g]) - 1 and result[g] == {1: 0, 2: 1, 3: -1}[r]
        if result[g] is None:
            assert len(hist[g]) == 30
    assert checked >= 2 * G                               # no game ends before its fourth ply
    assert res.num_inferences == 0 and res.avg_batch_size == 0
    assert abs(res.p1_winrate + res.p2_winrate + res.drawrate - 1.0) < 1e-9


def test_elo_rankings_with_a_minimax_anchor():
    _, elos, wm = V.compute_elo_rankings([V.Player.random(), V.Player.minimax(1, device=-1)], games=4, max_plies=20)
    assert np.allclose(elos, O.compute_elos(wm, 150.0), rtol=1e-6, atol=0)
    assert elos[0] == 150.0 and wm[1][0] + wm[0][1] == pytest.approx(1.0)


def raw_scores(par, depth, device=HOST):
    n = len(par)
    out = [np.full((n, L.MAX_MOVES), -7, np.int32) for _ in range(3)] + [np.full(n, -7, np.int32)]
    nodes = np.full(n, -7, np.int64)
    rc = L.lib.az_minimax_scores(device, par.ctypes.data_as(C.POINTER(L.AzPos)), n, depth, *[L.i32ptr(a) for a in out],
                                 nodes.ctypes.data_as(C.POINTER(C.c_int64)))
    return rc, out + [nodes]


def test_input_validation_writes_nothing():
    good = CH.positions_to_array([A.Position.startpos(), A.Position.startpos()])
    two_kings = good.copy()
    two_kings["bb"][1, 5] |= np.uint64(1 << 28)                        # a second white king on e4
    two_kings["bb"][1, 6] |= np.uint64(1 << 28)
    for par, depth, word in ((good, 0, "depth"), (good, 9, "depth"), (two_kings, 2, "king")):
        rc, outs = raw_scores(par, depth)
        assert rc < 0
        assert word in L.lib.az_last_error().decode()
        assert all((a == -7).all() for a in outs)
    rc, outs = raw_scores(good, 1)
    assert rc == 0 and outs[3].tolist() == [20, 20] and (outs[0][:, 20:] == -7).all()
    assert L.lib.az_minimax_scores(HOST, None, 1, 2, None, None, None, None, None) < 0
