"""Cases for the search-row tests (tests/test_searchrows.py, tests/test_gpu_search_rows.py): the roots, the
dispatch matrix of the network paths, and the closure that finds the oracle position behind every key of an
evaluation log.  The closure and the planes use the oracle only (oracle/oracle.py): no product code decides
what a logged row is compared with.

ROOTS are chosen so that the root evaluations alone (set_roots always evaluates a root) reach the corners of
to_tensor and of the legal-index write: both sides to move, every castling plane set and clear and a mixed set
of rights, an en-passant square for either side (one of them not capturable: the horizontal pin), clocks at
0.98 and 0.995, 218 edges, a promotion index listed four times, a single legal move, a three-piece board.
tests/test_searchrows.py asserts those conditions on the CPU.  Two roots are there twice, so that a position
is evaluated in two batch rows of one launch."""
import numpy as np

import oracle as O
from test_gpu_rules import SEARCH_ROOTS

START = "rnbqkbnr/pppppppp/8/8/8/8/PPPPPPPP/RNBQKBNR w KQkq - 0 1"


def history(fen, tours):
    """move indices of the (from, to) squares played from fen, by the oracle's move list"""
    p, hist = O.from_fen(fen), []
    for f, t in tours:
        moves, idx = O.legal_moves(p), O.legal_indices(p)
        at = [i for i, m in enumerate(moves) if (m[0], m[1]) == (f, t)]
        assert at, (fen, f, t)
        hist.append(int(idx[at[0]]))
        p = O.play_unchecked(p, moves[at[0]])
    return hist


# the roots of tests/test_gpu_rules.py (all have a legal move; the mate-in-one, 98-halfmove and 199-fullmove
# roots give terminal leaves, so a step's row count falls below the game count) ...
ROOTS = list(SEARCH_ROOTS)
# ... its two histories: knights out and back twice (the root has occurred twice), a shuffle at a 90-move clock
ROOTS += [(START, history(START, ((6, 21), (62, 45), (21, 6), (45, 62), (6, 21), (62, 45)))),
          ("4k3/8/8/8/8/8/8/R3K2R w - - 90 120", history("4k3/8/8/8/8/8/8/R3K2R w - - 90 120",
                                                        ((7, 15), (60, 59), (15, 7), (59, 60))))]
# ... and what the conditions of tests/test_searchrows.py still lacked
ROOTS += [
    ("r3k2r/8/8/8/8/8/8/R3K2R w Kq - 3 10", []),        # mixed rights: planes 12 and 15 set, 13 and 14 clear
    ("8/8/8/K2pP2r/8/8/8/7k w - d6 0 1", []),           # White to move with an ep square (not capturable: pinned)
    ("k7/8/1K6/8/8/8/8/7R b - - 0 1", []),              # one legal move (Kb8)
]
# ... and two roots again, in other batch rows (a pair's first board and the lone tail of a two-board launch, where
# the first copies are a pair's second and first board): without noise their searches are the same, so every
# position of theirs is logged twice and must carry the same bits both times
TWICE = (7, 8)                 # the middlegame with every castling right, and the 218 edges
ROOTS += [ROOTS[g] for g in TWICE]
assert len(ROOTS) == 17        # odd: a two-board launch has a lone tail


def root_position(fen, hist):
    """the oracle position of a root: fen with hist played"""
    p = O.from_fen(fen)
    for a in hist:
        m = O.index_to_move(int(a), p)
        assert m is not None, (fen, a)
        p = O.play_unchecked(p, m)
    return p


LAYERED = "conv3x3_kernel (per layer) + heads_kernel"
DIRECT = "tower32_kernel<%d> (f32, direct 3x3)"
WINO = "tower32w_kernel<%d> (f32, Winograd F(2x2,3x3) residual convs)"
SPLIT = "tower32w_kernel<%d> (f32, Winograd F(2x2,3x3) residual convs, split-f16 MFMA products)"
BF16 = "tower_kernel<%d> (bf16, direct 3x3)"
FP8 = "tower8_kernel<%d> (MX-fp8 e4m3, direct 3x3)"
NET_ENV = ("AZ_FUSED_TOWER", "AZ_WINOGRAD", "AZ_WINO_SPLIT16", "AZ_WINO_DERIVE", "AZ_WINO_ROWS", "AZ_WINO_VROWS",
           "AZ_WINO_BOARDS")
BLOCKS = 2


def _paths():
    """(id, dtype, filters, env, kernel name, persistent kernel supported, form) for every search instantiation
    the dispatch reaches: tower.hip tower_forward / sims_persistent, tower8.hip tower8_forward and the unfused
    branch of search.hip (encode_rows_kernel, conv3x3 per layer, heads_kernel<F, T, true>).  The persistent
    kernel exists for the f32 Winograd towers and the bf16 64-filter tower, fused only (tower.hip
    sims_persistent_supported, search.hip use_persistent).  form: the split-f16 tower's accessors
    (streamed points, accumulators, shared V rows, boards), which the kernel name does not tell apart."""
    out = [("f32-32-direct", "f32", 32, {}, DIRECT, False, None)]
    for f in (64, 128):
        out += [("f32-%d-wino" % f, "f32", f, {}, WINO, True, None),
                ("f32-%d-split16" % f, "f32", f, {"AZ_WINO_SPLIT16": "2"}, SPLIT, True, (16, 16, 0, 1)),
                ("f32-%d-direct" % f, "f32", f, {"AZ_WINOGRAD": "0"}, DIRECT, False, None)]
    out += [("f32-256-boards2", "f32", 256, {}, SPLIT, True, (12, 8, 1, 2)),
            ("f32-256-boards1", "f32", 256, {"AZ_WINO_BOARDS": "1"}, SPLIT, True, (12, 8, 1, 1)),
            ("f32-256-vrows0", "f32", 256, {"AZ_WINO_VROWS": "0"}, SPLIT, True, (12, 8, 0, 1)),
            ("f32-256-rows0", "f32", 256, {"AZ_WINO_ROWS": "0"}, SPLIT, True, (12, 16, 0, 1)),
            ("f32-256-derive0", "f32", 256, {"AZ_WINO_DERIVE": "0"}, SPLIT, True, (16, 16, 0, 1)),
            ("f32-256-wino", "f32", 256, {"AZ_WINO_SPLIT16": "0"}, WINO, True, None),
            ("f32-256-direct", "f32", 256, {"AZ_WINOGRAD": "0"}, DIRECT, False, None)]
    out += [("f32-%d-layer" % f, "f32", f, {"AZ_FUSED_TOWER": "0"}, LAYERED, False, None) for f in (32, 64, 128, 256)]
    out += [("bf16-%d" % f, "bf16", f, {}, BF16, f == 64, None) for f in (32, 64, 128, 256)]
    out += [("bf16-%d-layer" % f, "bf16", f, {"AZ_FUSED_TOWER": "0"}, LAYERED, False, None) for f in (32, 64, 128, 256)]
    out += [("fp8-%d" % f, "fp8", f, {}, FP8, False, None) for f in (128, 256)]
    return [(i, d, f, e, k % f if "%d" in k else k, p, form) for i, d, f, e, k, p, form in out]


PATHS = _paths()
PATH = {p[0]: p for p in PATHS}
LEAF_PATHS = ("f32-256-layer", "f32-256-boards2", "bf16-64")      # leaves = 4
NOISE_PATHS = ("f32-128-wino", "bf16-256")                          # apply_noise = True

_children = {}      # fen key -> {child key: child RefPos}, over the distinct legal indices


def children(key, p):
    """the positions one oracle move below p (key = O.fen_key(p)), by key; computed once per key"""
    if key not in _children:
        acts = np.unique(O.legal_indices(p)).astype(np.int32)
        kids = {}
        if len(acts):
            par = (O.RefPos * len(acts))(*([p] * len(acts)))
            r = O.rules_batch(par, acts)
            for i in range(len(acts)):
                kids.setdefault(int(r["fen_key"][i]), O.RefPos.from_buffer_copy(r["child"][i]))
        _children[key] = kids
    return _children[key]


def closure(roots, logged_keys):
    """{fen key: oracle position} for every logged key: the roots, then the children whose key is logged, and
    so on down.  Raises if a logged key is not reached: no row may be left out."""
    logged = set(int(k) for k in logged_keys)
    known, todo = {}, []
    for fen, hist in roots:
        p = root_position(fen, hist)
        todo.append((int(O.fen_key(p)), p))
    while todo:
        k, p = todo.pop()
        if k in known or k not in logged:
            continue
        known[k] = p
        todo += [(ck, cp) for ck, cp in children(k, p).items() if ck in logged and ck not in known]
    missing = logged - set(known)
    if missing:
        raise KeyError("%d logged keys are no root and no child of a logged position: %s"
                       % (len(missing), sorted(missing)[:4]))
    return known


def oracle_planes(positions):
    """O.to_tensor of every position, [n, 19 * 64] float32"""
    return np.stack([O.to_tensor(p) for p in positions]).reshape(len(positions), 19 * 64).astype(np.float32)


def synthetic_search_keys(fen, hist, sims=24, c_puct=3.0):
    """The keys the oracle's search evaluates from one root with its synthetic evaluator, noise off
    (oracle/mcts_ref.c mct_simulation restated on O.synth_eval and O.Game, in float32), and the root's visits:
    tests/test_searchrows.py checks the visits against ref_search_from, so the keys are that search's."""
    f32 = np.float32

    def game(path):
        g = O.Game(O.from_fen(fen))
        r = 0
        for a in list(hist) + path:
            r = g.play_index(int(a))
        return g, r

    class Node:
        def __init__(self, path):
            g, _ = game(path)
            self.path, pos = path, g.position
            self.moves = O.legal_indices(pos)
            self.policy, self.value = O.synth_eval(pos)
            self.visits, self.scores, self.kids = np.zeros(4096, f32), np.zeros(4096, f32), {}
            keys.append(int(O.fen_key(pos)))

    def simulate(t):
        total = f32(0)
        for v in t.visits:               # sequential float32 sum, as the oracle's
            total = f32(total + v)
        root = np.sqrt(f32(total + f32(1)))
        m = t.moves
        u = (f32(c_puct) * t.policy[m]) * root / (f32(1) + t.visits[m])
        q = np.where(t.visits[m] > 0, t.scores[m] / np.maximum(t.visits[m], f32(1)), f32(0)).astype(f32)
        a = int(m[int(np.argmax((q + u).astype(f32)))])        # the first of equal maxima: strict >
        if a in t.kids:
            value = -simulate(t.kids[a])
        else:
            _g, r = game(t.path + [a])
            if r == 0:
                t.kids[a] = Node(t.path + [a])
                value = -f32(t.kids[a].value)
            else:
                value = f32(0) if r == DRAW else f32(1)
        t.scores[a] = f32(t.scores[a] + value)
        t.visits[a] = f32(t.visits[a] + f32(1))
        return value

    keys = []
    root = Node([])
    for _ in range(sims):
        simulate(root)
    return keys, root.visits


DRAW = 1        # oracle/az_oracle.h REF_DRAW: play_index's result for a drawn game (0: the game goes on)
