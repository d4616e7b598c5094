"""tests/searchrows.py on the CPU: the roots of the search-row tests reach the corners of to_tensor and of the
legal-index write by themselves (a root's evaluation is always logged), the dispatch matrix holds the entries
the tests are specified on, and the closure finds every key of a search and refuses a foreign one.  Everything
is computed from the oracle's planes and move lists."""
import numpy as np
import pytest

import oracle as O
import searchrows as S

POS = [S.root_position(fen, hist) for fen, hist in S.ROOTS]
PLANES = S.oracle_planes(POS).reshape(len(POS), 19, 64)
MOVES = [O.legal_indices(p) for p in POS]
WHITE = np.array([p.turn == 0 for p in POS])


def test_roots_have_moves_and_an_odd_count():
    assert 13 <= len(S.ROOTS) <= 17 and len(S.ROOTS) % 2 == 1
    assert all(len(m) >= 1 and O.outcome(p) == 0 for m, p in zip(MOVES, POS))
    # distinct but for the two roots that are there twice, which are a whole pair of boards and more apart
    assert len({int(O.fen_key(p)) for p in POS}) == len(POS) - len(S.TWICE)
    for k, g in enumerate(S.TWICE):
        assert S.ROOTS[len(POS) - len(S.TWICE) + k] == S.ROOTS[g] and len(POS) - len(S.TWICE) + k - g >= 2
    assert max(len(set(MOVES[g].tolist())) for g in S.TWICE) == 218


def test_both_sides_to_move():
    assert WHITE.any() and (~WHITE).any()
    assert {p.turn for p in POS} == {0, 1}


def test_castling_planes_set_clear_and_mixed():
    rights = PLANES[:, 12:16]
    assert np.all((rights == 0) | (rights == 1)) and np.all(rights.min(2) == rights.max(2))
    r = rights[:, :, 0]
    for k in range(4):
        assert (r[:, k] == 1).any() and (r[:, k] == 0).any(), 12 + k
    assert any(0 < row.sum() < 4 and row[0] != row[1] and row[2] != row[3] for row in r)      # such as Kq


def test_en_passant_plane_for_both_sides_and_the_pin():
    ep = PLANES[:, 16].sum(1)
    assert set(ep.tolist()) == {0.0, 1.0}
    assert (ep[WHITE] == 1).any() and (ep[~WHITE] == 1).any()
    # the square is in the plane although the capture is illegal (the horizontal pin): FEN's pseudo-legal square
    assert any(e == 1 and O.legal_ep(p) < 0 for e, p in zip(ep, POS))
    assert any(e == 1 and O.legal_ep(p) >= 0 for e, p in zip(ep, POS))


def test_clock_planes():
    half, full = PLANES[:, 17], PLANES[:, 18]
    assert np.all(half.min(1) == half.max(1)) and np.all(full.min(1) == full.max(1))
    assert (half[:, 0] >= 0.98).any() and (half[:, 0] == 0).any()
    assert (full[:, 0] >= 0.99).any()


def test_edge_count_corners():
    distinct = [len(set(m.tolist())) for m in MOVES]
    assert max(distinct) == 218
    assert any(len(m) == 1 for m in MOVES)
    assert min(distinct) == 1 and sum(20 <= d <= 40 for d in distinct) < len(distinct) // 2


def test_a_promotion_index_is_listed_four_times():
    four = [m for m in MOVES if 4 in np.unique(m, return_counts=True)[1]]
    assert four
    # and it is a queen promotion: a pawn move to the last rank (index = 64 from + to, from the mover's side)
    m = four[0]
    idx = int(np.unique(m)[np.unique(m, return_counts=True)[1] == 4][0])
    p = POS[[i for i, mm in enumerate(MOVES) if mm is m][0]]
    frm, to, promo, _kind = O.index_to_move(idx, p)
    assert promo != 0 and (to // 8 in (0, 7))


def test_a_board_with_few_pieces():
    pieces = PLANES[:, :12].sum((1, 2))
    assert pieces.min() <= 4 and pieces.max() >= 30


def test_dispatch_matrix_holds_the_specified_entries():
    have = {(d, f, tuple(sorted(e.items()))) for _i, d, f, e, _k, _p, _form in S.PATHS}
    want = [("f32", 32, {})]
    want += [("f32", f, e) for f in (64, 128) for e in ({}, {"AZ_WINO_SPLIT16": "2"}, {"AZ_WINOGRAD": "0"})]
    want += [("f32", 256, e) for e in ({}, {"AZ_WINO_BOARDS": "1"}, {"AZ_WINO_VROWS": "0"}, {"AZ_WINO_ROWS": "0"},
                                       {"AZ_WINO_DERIVE": "0"}, {"AZ_WINO_SPLIT16": "0"}, {"AZ_WINOGRAD": "0"})]
    want += [("f32", 32, {"AZ_FUSED_TOWER": "0"}), ("f32", 256, {"AZ_FUSED_TOWER": "0"})]
    want += [("bf16", f, {}) for f in (32, 64, 128, 256)] + [("bf16", 64, {"AZ_FUSED_TOWER": "0"})]
    want += [("fp8", 128, {}), ("fp8", 256, {})]
    for d, f, e in want:
        assert (d, f, tuple(sorted(e.items()))) in have, (d, f, e)
    assert len({p[0] for p in S.PATHS}) == len(S.PATHS)
    assert all(set(p[3]) <= set(S.NET_ENV) for p in S.PATHS)
    # the persistent kernel: the fused f32 Winograd towers and the fused bf16 64-filter tower
    for _i, d, f, e, k, pers, _form in S.PATHS:
        assert pers == (k.startswith("tower32w_kernel") or (k.startswith("tower_kernel") and f == 64)), k
    kinds = {S.PATH[i][4].split("<")[0].split(" ")[0] for i in S.LEAF_PATHS}
    assert "conv3x3_kernel" in kinds and S.PATH["f32-256-boards2"][6][3] == 2 and "bf16-64" in S.LEAF_PATHS
    assert len(S.NOISE_PATHS) == 2


SYNTH = {}


def synth(g):
    if g not in SYNTH:
        SYNTH[g] = S.synthetic_search_keys(*S.ROOTS[g])
    return SYNTH[g]


@pytest.mark.parametrize("g", range(len(S.ROOTS)))
def test_synthetic_search_restatement_is_the_oracles(g):
    """the Python restatement that yields the evaluated keys visits what ref_search_from visits"""
    fen, hist = S.ROOTS[g]
    keys, visits = synth(g)
    rv, _ri, _rd, evals = O.search_game(O.make_cfg(sims=24, noise=False, eval_kind=0), hist, start=O.from_fen(fen))
    assert np.array_equal(visits, rv), fen
    assert len(keys) == evals


def test_closure_returns_every_key_of_the_synthetic_search():
    keys = [k for g in range(len(S.ROOTS)) for k in synth(g)[0]]
    assert len(keys) < 25 * len(S.ROOTS)            # terminal leaves: some simulations evaluate nothing
    known = S.closure(S.ROOTS, keys)
    assert set(known) == set(keys)
    for k, p in known.items():
        assert int(O.fen_key(p)) == k
    planes = S.oracle_planes([known[k] for k in sorted(known)])
    assert planes.shape == (len(known), 19 * 64) and planes.dtype == np.float32
    again = S.closure(S.ROOTS, keys[::-1])          # the children cache changes nothing
    assert set(again) == set(known)


def test_closure_raises_on_a_key_outside_the_tree():
    keys = synth(0)[0]
    foreign = O.fen_key(O.from_fen("8/8/8/8/8/8/8/K1k5 w - - 0 1"))
    with pytest.raises(KeyError):
        S.closure(S.ROOTS, keys + [foreign])
    # a position two plies below the last logged one: its parent is not logged, so it is not reached
    p = S.root_position(*S.ROOTS[7])
    kid = next(iter(S.children(int(O.fen_key(p)), p).items()))
    grand = next(iter(S.children(*kid).items()))
    with pytest.raises(KeyError):
        S.closure(S.ROOTS, [int(O.fen_key(p)), grand[0]])
    assert set(S.closure(S.ROOTS, [int(O.fen_key(p)), kid[0], grand[0]])) == {int(O.fen_key(p)), kid[0], grand[0]}
