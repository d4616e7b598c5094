"""The batched negamax kernels (az_minimax_scores on a GPU) against the host path -- moves,
promotion roles, scores and negamax call counts, bit for bit -- and, independently of the host path,
against the Python restatement of chess.rs:248-322 (tests/minimax_ref.py); the same results at any
frontier capacity (chunked batches, an earlier split ply); and the arena's MiniMax player on the GPU."""
import numpy as np
import pytest

import azchess as A
import oracle as O
from azchess import chess as CH
from azchess import validation as V

import minimax_ref as R

pytestmark = pytest.mark.gpu

KIWIPETE = R.FENS["kiwipete"]


def position(fen):
    return A.Position.startpos() if fen is None else A.Position.from_fen(fen)


def table():
    return [position(f) for _, f in R.TABLE]


def playouts():
    return [position(f) for f in R.playout_fens()]


_host = {}


def host(key, positions, depth):
    """the host path's answer, computed once per case and shared"""
    if (key, depth) not in _host:
        _host[key, depth] = CH.minimax_scores(positions, depth, CH.DEVICE_HOST)
    return _host[key, depth]


def assert_equal(got, ref, what):
    (ge, gn), (re, rn) = got, ref
    assert len(ge) == len(re)
    for i, (g, r) in enumerate(zip(ge, re)):
        for a, b, field in zip(g, r, ("moves", "promo", "scores")):
            assert np.array_equal(a, b), (what, i, field, a.tolist(), b.tolist())
    assert np.array_equal(gn, rn), (what, gn.tolist(), rn.tolist())


@pytest.mark.parametrize("depth", [1, 2, 3, 4])
def test_table_equals_host_path(require_gpu, depth):
    assert_equal(CH.minimax_scores(table(), depth), host("table", table(), depth), depth)


def test_kiwipete_depth_4_equals_host_path(require_gpu):
    got = CH.minimax_scores([position(KIWIPETE)], 4)
    assert_equal(got, host("kiwipete", [position(KIWIPETE)], 4), "kiwipete")
    assert int(got[1][0]) == 48 + 2039 + 97862 + 4085603             # perft 1..4: no line ends early


def test_playout_positions_depth_3_equal_host_path(require_gpu):
    assert_equal(CH.minimax_scores(playouts(), 3), host("playouts", playouts(), 3), "playouts")


def test_table_depth_2_equals_python_reference(require_gpu):
    entries, nodes = CH.minimax_scores(table(), 2)
    for i, (name, fen) in enumerate(R.TABLE):
        mv, pr, sc, calls = R.scores_of_fen(fen, 2)
        assert np.array_equal(entries[i][0], mv) and np.array_equal(entries[i][1], pr), name
        assert np.array_equal(entries[i][2], sc) and int(nodes[i]) == calls, name


@pytest.mark.parametrize("capacity", ["256", "4096"])
def test_results_do_not_depend_on_the_frontier_capacity(require_gpu, monkeypatch, capacity):
    """256 nodes: the 48-position batch goes in chunks and every tree is searched depth-first from
    its first ply; 4096: kiwipete's third ply (97,862 nodes) no longer fits, so the split is a ply
    earlier than with the default buffer"""
    monkeypatch.delenv("AZ_MINIMAX_FRONTIER", raising=False)
    kiwi = CH.minimax_scores([position(KIWIPETE)], 4)
    batch = CH.minimax_scores(playouts(), 3)
    assert_equal(CH.minimax_scores([position(KIWIPETE)], 4), kiwi, "second default call")
    assert_equal(CH.minimax_scores(playouts(), 3), batch, "second default call")
    monkeypatch.setenv("AZ_MINIMAX_FRONTIER", capacity)
    assert_equal(CH.minimax_scores([position(KIWIPETE)], 4), kiwi, capacity)
    assert_equal(CH.minimax_scores(playouts(), 3), batch, capacity)


def test_arena_minimax_on_the_gpu(require_gpu):
    G, sims, seed, depth = 6, 8, 3, 3
    res, hist, result = V.evaluate(V.Player.minimax(depth), V.Player.mcts(None), games=G, sims=sims, seed=seed,
                                   max_plies=24, record=True)
    cfg = O.make_cfg(sims=sims, noise=False, seed=0, eval_kind=0)
    for g in range(G):
        og, state = O.Game(), A.GameState()
        for ply, a in enumerate(hist[g]):
            u = V.choice_uniform(seed, g, ply)
            if (g % 2 == 0) == (ply % 2 == 0):                         # MiniMax moves: the host path
                assert a == CH.get_best_move(state.position, depth, u, device=CH.DEVICE_HOST), (g, ply)
            else:                                                      # MCTS moves: the oracle's search
                _, imp, _, _ = O.search_game(cfg, hist[g][:ply], noise=False)
                assert a == O.arena_choose(imp, og.position.fullmoves, 15, u), (g, ply)
            r = og.play_index(a)
            assert r >= 0 and int(A.play_move(state, a)) == r, (g, ply)
            if r != 0:
                assert ply == len(hist[g]) - 1 and result[g] == {1: 0, 2: 1, 3: -1}[r]
    # the MCTS player's batches only: at most one search per ply
    assert 0 < res.num_inferences <= 24 * (sims + 1) and res.num_inferences % (sims + 1) == 0
    assert abs(res.p1_winrate + res.p2_winrate + res.drawrate - 1.0) < 1e-9
