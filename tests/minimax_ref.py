"""The MiniMax bot's search (chess.rs:248-322) restated in Python over the oracle's rules: the
reference of tests/test_minimax.py and tests/test_gpu_minimax.py.  About 30 k nodes/s, so depths
of 3 or less; results are cached per (FEN, depth) and shared between the tests of a session."""
import functools

import numpy as np

import oracle as O

VALUE = {1: 100, 2: 320, 3: 330, 4: 500, 5: 900, 6: 0}    # chess.rs:248-252; kings count 0
MATE_SCORE = 20000

# (name, FEN or None for the start position): the issue's table
TABLE = [
    ("startpos", None),
    ("kiwipete", "r3k2r/p1ppqpb1/bn2pnp1/3PN3/1p2P3/2N2Q1p/PPPBBPPP/R3K2R w KQkq - 0 1"),
    ("pos4", "r3k2r/Pppp1ppp/1b3nbN/nP6/BBP1P3/q4N2/Pp1P2PP/R2Q1RK1 w kq - 0 1"),
    ("mate_in_1", "6k1/5ppp/8/8/8/8/5PPP/R5K1 w - - 0 1"),
    ("mate_in_2", "6k1/5ppp/8/8/8/8/1R3PPP/R5K1 w - - 0 1"),
    ("stalemate_promo", "8/5P1k/5K2/8/8/8/8/8 w - - 0 1"),
    ("promo_two_mates", "8/5P1p/6pk/6p1/6P1/7K/8/8 w - - 0 1"),
    ("capture_into_kvk", "8/8/8/8/k3r3/3K4/8/8 w - - 0 1"),
    ("en_passant", "8/8/8/2k5/3Pp3/8/8/4K3 b - d3 0 1"),
    ("castling", "r3k2r/8/8/8/8/8/8/R3K2R w KQkq - 0 1"),
    ("black_promo", "8/8/8/8/8/2k5/1p6/7K b - - 0 1"),
]
# The issue's own "Black promoting" FEN has the white king on a1, in check from the b2 pawn with
# Black to move: shakmaty's from_setup, the engine's from_fen and az_minimax_scores' required
# setup_error all refuse it (its 15 entries count four captures of the king).  The table keeps the
# case with the king on h1 -- 4 promotion entries and 7 king moves -- and the tests pin the refusal.
ISSUE_BLACK_PROMO_FEN = "8/8/8/8/8/2k5/1p6/K7 b - - 0 1"
FENS = dict(TABLE)


def ref_position(fen):
    return O.startpos() if fen is None else O.from_fen(fen)


def evaluate_material(p):           # chess.rs:255-266
    s = 0
    for c in p.sq:
        if c:
            v = VALUE[abs(c)]
            s += v if (c > 0) == (p.turn == 0) else -v
    return s


def negamax(p, depth, calls):       # chess.rs:268-295
    calls[0] += 1
    oc = O.outcome(p)
    if depth == 0 or oc != 0:
        if oc != 0:
            return 0 if oc == 1 else -MATE_SCORE - depth
        return evaluate_material(p)
    best = -(1 << 31)
    for m in O.legal_moves(p):
        best = max(best, -negamax(O.play_unchecked(p, m), depth - 1, calls))
    return best


def scores_of(p, depth):
    """get_best_move's loop (chess.rs:298-319) on a RefPos: (moves as move_to_index, promo as
    0 / 1 N / 2 B / 3 R / 4 Q, scores, negamax calls), in legal_moves() order."""
    calls = [0]
    mv, pr, sc = [], [], []
    for m in O.legal_moves(p):
        mv.append(O.move_to_index(m, p.turn))
        pr.append(m[2] - 1 if m[2] else 0)                # the oracle's promo codes: N 2, B 3, R 4, Q 5
        sc.append(-negamax(O.play_unchecked(p, m), depth - 1, calls))
    return np.array(mv, np.int32), np.array(pr, np.int32), np.array(sc, np.int32), calls[0]


@functools.lru_cache(maxsize=None)
def scores_of_fen(fen, depth):
    return scores_of(ref_position(fen), depth)


def best_entry(scores, u):
    """best_moves.choose (chess.rs:304-321) at the uniform u: the min(floor(u * ties), ties - 1)-th
    of the entries with the maximal score, in list order (the product in float32)."""
    ties = np.flatnonzero(scores == scores.max())
    return int(ties[min(int(np.floor(np.float32(u) * np.float32(len(ties)))), len(ties) - 1)])


@functools.lru_cache(maxsize=None)
def playout_fens():
    """48 positions at evenly spaced indices of the oracle's seeded random playouts, as FENs"""
    parents, _ = O.random_playouts(7, 4, 120, 2000)
    idx = np.linspace(0, len(parents) - 1, 48).astype(int)
    return tuple(O.to_fen(parents[i]) for i in idx)
