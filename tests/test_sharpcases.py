"""The sharp search cases on the host: every reference of tests/test_gpu_sharp_search.py computed once
(functools.lru_cache; the GPU file imports them from here), the conditions that make each case worth
running -- stated from the references alone -- and the two references against each other: for every K = 1,
reuse-off case the numpy restatement (tests/leafpar_ref.py) and the C oracle (O.search_game over an O.Replay
of the rows the restatement asked for) agree bit for bit.  No GPU.

Run with -s for one line per case: depth, shared leaves, ties, wide nodes, kept nodes."""
import contextlib
import functools
import types

import numpy as np
import pytest

import azchess as A
import leafpar_ref as L
import oracle as O
import sharpcases as S
import treereuse_ref as T
from test_oracle_search_api import move_index

F = np.float32
SEED = 11
WIDE_FEN = "3q1q1q/k7/2q5/8/8/5Q2/6K1/1QQ1Q3 w - - 0 1"           # 8 queens, nobody in check: nodes of > 64 moves below it
Q218_FEN = "R6R/3Q4/1Q4Q1/4Q3/2Q4Q/Q4Q2/pp1Q4/kBNN1KB1 w - - 0 1"   # 218 legal moves (tests/test_gpu_rules.py)
SHUFFLE = (("g1", "f3"), ("g8", "f6"), ("f3", "g1"), ("f6", "g8"))   # the start position, seen twice


@functools.lru_cache(maxsize=None)
def shuffle_history():
    g, h = O.Game(), []
    for frm, to in SHUFFLE:
        h.append(move_index(g.position, frm, to))
        assert g.play_index(h[-1]) == 0
    return tuple(h)


@functools.lru_cache(maxsize=None)
def last_line_history(plies=5):
    """the first plies of the `last` family's one-hot line from the start position: a root from which that
    line repeats, for the third time, a position that the history before the root holds too"""
    g, h = O.Game(), []
    for _ in range(plies):
        h.append(S.distinct(O.legal_indices(g.position))[-1])
        assert g.play_index(h[-1]) == 0
    return tuple(h)


def root(name):
    """(FEN or None = the start position, history) of a named root"""
    return {"start": (None, ()), "shuffle": (None, shuffle_history()), "wide": (WIDE_FEN, ()),
            "lastline": (None, last_line_history())}[name]


def engine_roots(names):
    """(starts, histories) for BatchedSearch.set_roots(histories, start=starts)"""
    fens = [root(n)[0] for n in names]
    return ([A.Position.startpos() if f is None else A.Position.from_fen(f) for f in fens],
            [list(root(n)[1]) for n in names])


# name: (family, sims, roots); one engine handle per case, root g of the list is game g of the handle
STEP_CASES = {
    "hashed": ("hashed", 200, ("start", "wide", "shuffle")),
    "first": ("first", 200, ("start", "shuffle")),
    "last": ("last", 64, ("start", "lastline")),
    "zeros64": ("zeros", 64, ("start", "wide", "shuffle")),
    "zeros200": ("zeros", 200, ("wide", "start")),
    "uniform": ("uniform", 64, ("start", "wide")),
    "tiny": ("tiny", 64, ("start", "wide")),
    "nanmix64": ("nanmix", 64, ("start", "shuffle", "wide")),
    "nanmix200": ("nanmix", 200, ("wide", "start")),
    "allnan": ("allnan", 64, ("start", "wide")),
}
# nanmix searches in which some node's every edge ends up NaN (a NaN value backed up into each W): the C
# oracle aborts there, so these go to the numpy restatement only, as allnan does
RESTATEMENT_ONLY = {("nanmix64", "shuffle"), ("nanmix200", "wide"), ("nanmix200", "start")}
NOISE_CASES = ("hashed", "zeros64", "zeros200", "nanmix64", "nanmix200")
# name: (family, sims, K, roots)
LEAF_CASES = {
    "hashed_k4": ("hashed", 400, 4, ("start",)),
    "first_k8": ("first", 600, 8, ("start",)),
    "allnan_k4": ("allnan", 64, 4, ("start", "wide")),
}
LEAF_CASES.update({"%s_k%d" % (f, k): (f, 64, k, ("start", "wide")) for f in ("uniform", "zeros", "nanmix")
                   for k in (4, 8)})
REUSE_SIMS, REUSE_PLIES = 160, 4
REUSE_CASES = {"hashed": ("start", "shuffle"), "nanmix": ("start", "shuffle"), "zeros": ("start", "shuffle")}


# ------------------------------------------------------------------ what the selections met
def counted_pick(tally):
    """leafpar_ref.pick with its loop copied: the same edge, and counts of what the selection met"""
    def pick(node, c_edge, c_puct):
        c = np.asarray(c_edge, np.int64)
        n = node.N + c
        w = node.W - c.astype(F)
        sq = np.sqrt(F(int(node.N.sum()) + int(c.sum()) + 1))
        nf = n.astype(F)
        with np.errstate(all="ignore"):
            u = F(c_puct) * node.P * sq / (F(1.0) + nf)
            q = np.where(n > 0, w / np.where(n > 0, nf, F(1.0)), F(0.0)).astype(F)
            v = q + u
        best, bpos, equal = F(-np.inf), 0, 0
        for e in range(len(v)):
            if v[e] > best:
                best, bpos, equal = v[e], e, 1
            elif v[e] == best:
                equal += 1
        wide = len(v) > 64
        tally.selections += 1
        tally.wide += wide
        if not best > F(-np.inf):                       # nothing beat -inf: the first edge
            tally.fallback += 1
        elif equal >= 2:
            tally.ties += 1
            tally.deep_ties += node.depth > 0
            tally.wide_ties += wide
        tally.inf_taken += bool(np.isposinf(node.P[bpos]))
        return bpos
    return pick


def new_tally():
    return types.SimpleNamespace(selections=0, ties=0, deep_ties=0, wide=0, wide_ties=0, fallback=0, inf_taken=0)


@contextlib.contextmanager
def counting(tally):
    old = L.pick, T.pick
    L.pick = T.pick = counted_pick(tally)
    try:
        yield
    finally:
        L.pick, T.pick = old


def wide_nodes(log):
    """evaluated positions with more than 64 distinct legal moves"""
    return sum(1 for idx, _, _ in log.values() if len(idx) > 64)


# ------------------------------------------------------------------ the references, computed once
@functools.lru_cache(maxsize=None)
def search_ref(family, rootname, sims, K, noise, game):
    """leafpar_ref.search of one root as game `game` of its handle -> namespace(out = (visits, improved,
    depth, shared, evals), counts, tally, log, and the arguments)"""
    fen, hist = root(rootname)
    start = None if fen is None else O.from_fen(fen)
    log, tally, counts = {}, new_tally(), {}
    key = O.lib().ref_stream_key(SEED, game, len(hist), 0) if noise else None
    with counting(tally):
        out = L.search(start, list(hist), (sims, K), S.ref_evaluator(family, log), key, counts=counts)
    return types.SimpleNamespace(out=out, visits=out[0], improved=out[1], depth=out[2], shared=out[3], evals=out[4],
                                 counts=counts, tally=tally, log=log, start=start, hist=hist, key=key, sims=sims,
                                 family=family, root=rootname, K=K, noise=noise, wide=wide_nodes(log))


def step_refs(name, noise=False):
    family, sims, roots = STEP_CASES[name]
    return [search_ref(family, r, sims, 1, noise, g) for g, r in enumerate(roots)]


def leaf_refs(name):
    family, sims, K, roots = LEAF_CASES[name]
    return [search_ref(family, r, sims, K, False, g) for g, r in enumerate(roots)]


@functools.lru_cache(maxsize=None)
def reuse_refs(family):
    """treereuse_ref.stepwise of the family's roots, per game, with what its selections met"""
    tally = new_tally()
    with counting(tally):
        recs = [T.stepwise(list(root(r)[1]), g, REUSE_PLIES, REUSE_SIMS, None, S.ref_evaluator(family))
                for g, r in enumerate(REUSE_CASES[family])]
    return recs, tally


@functools.lru_cache(maxsize=None)
def reuse_selfplay_ref(family, game, seed, sims, plies, temp_moves=15):
    """treereuse_ref.selfplay_game's loop (training.rs:294-338 with tree reuse, noise on) stopped after
    `plies` plies -> [per ply: Search.run()'s dict + action and result (of playing it: 0 = the game goes on)]"""
    key = lambda p: T.stream_key(seed, game, p)
    s = T.Search((), S.ref_evaluator(family), sims, key(0))
    out = []
    for ply in range(plies):
        rec = s.run()
        late = s.game.position.fullmoves >= temp_moves
        rec["action"] = s.last_max() if late else s.weighted(T.stream_key(seed, game, ply, 1))
        rec["result"] = s.advance(rec["action"], key(ply + 1))
        out.append(rec)
        if rec["result"] != 0:
            break
    return out


def line(r, tag=""):
    t = r.tally
    print("%-22s %-8s %-7s sims %3d K %d noise %d: depth %3d shared %3d evals %3d new_terminal %2d known_terminal %3d "
          "ties %3d (below the root %3d, wide %3d) wide nodes %3d inf taken %3d fallback %3d"
          % (tag, r.family, r.root, r.sims, r.K, r.noise, r.depth, r.shared, r.evals, r.counts["new_terminal"],
             r.counts["known_terminal"], t.ties, t.deep_ties, t.wide_ties, r.wide, t.inf_taken, t.fallback))


# ------------------------------------------------------------------ the adapters
def test_both_adapters_hand_out_the_same_rows():
    """the engine-side adapter (Position.fen_key / legal_indices) and the reference-side one (O.fen_key /
    O.legal_indices) give bit-identical rows and values along the `last` line and on the wide roots"""
    positions = []
    for fen in (None, WIDE_FEN, Q218_FEN):
        g = O.Game(None if fen is None else O.from_fen(fen))
        p = A.Position.startpos() if fen is None else A.Position.from_fen(fen)
        for _ in range(12):
            positions.append((g.position, p))
            a = S.distinct(O.legal_indices(g.position))[-1]
            if g.play_index(a) != 0:
                break
            p = p.play(a)
    assert len(positions) >= 20
    for family in S.FAMILIES:
        ref, gpu = S.ref_evaluator(family), S.gpu_evaluator(family)
        pol, val = gpu([p for _, p in positions])
        for k, (rp, _) in enumerate(positions):
            row, v = ref(rp)
            assert np.array_equal(row.view(np.uint32), pol[k].view(np.uint32)), (family, k)
            assert F(v).view(np.uint32) == val[k].view(np.uint32), (family, k)


def test_family_rows_are_what_the_table_says():
    pos = O.from_fen(Q218_FEN)
    idx = S.distinct(O.legal_indices(pos))
    assert len(idx) > 64
    legal = np.zeros(4096, bool)
    legal[idx] = True
    for family in ("first", "last", "hashed"):
        row, _ = S.ref_evaluator(family)(pos)
        assert row[legal].sum() == 1.0 and np.count_nonzero(row[legal]) == 1 and np.all(row[~legal] == 7.0)
    assert S.ref_evaluator("first")(pos)[0][idx[0]] == 1.0 and S.ref_evaluator("last")(pos)[0][idx[-1]] == 1.0
    row, v = S.ref_evaluator("zeros")(pos)
    assert not row[legal].any() and float(v) in S.GRID5
    row, v = S.ref_evaluator("uniform")(pos)
    assert np.all(row[legal] == F(1.0) / F(len(idx))) and v == 0.0
    row, v = S.ref_evaluator("tiny")(pos)
    assert np.all(row[legal] > 0) and np.all(row[legal] < np.finfo(F).tiny) and v == 0.0      # subnormal, not 0
    row, _ = S.ref_evaluator("nanmix")(pos)
    assert np.isnan(row[~legal]).all() and not np.isnan(row[idx[0]])
    assert np.isnan(row[legal]).any() and np.isposinf(row[legal]).any() and np.isfinite(row[legal]).any()
    row, v = S.ref_evaluator("allnan")(pos)
    assert np.isnan(row).all() and np.isnan(v)


# ------------------------------------------------------------------ the cases' conditions
def test_deep_line():
    """depth >= 130: backup_game's loop over path levels 64 and up takes two strides (k = lane + 64 and
    k = lane + 128); a chain: every simulation made a node"""
    r = step_refs("hashed")[0]
    line(r, "deep line")
    assert r.depth >= 130
    assert r.evals == r.sims and r.counts["new_terminal"] == r.counts["known_terminal"] == 0     # sims + 1 nodes
    for g, r in enumerate(step_refs("hashed")[1:], 1):
        line(r, "deep line, game %d" % g)


def test_deep_mate():
    r = step_refs("first")[0]
    line(r, "deep mate")
    assert r.depth >= 65 and r.counts["new_terminal"] >= 1 and r.counts["known_terminal"] >= 20
    line(step_refs("first")[1], "deep mate, game 1")


@pytest.mark.parametrize("name", ["hashed_k4", "first_k8"])
def test_deep_leaf_parallel(name):
    r = leaf_refs(name)[0]
    line(r, "deep leaf-parallel")
    assert r.depth >= 65 and 2 * r.shared >= r.sims


def placement(pos):
    """what a repetition compares: the FEN without its two clocks"""
    return " ".join(O.to_fen(pos).split()[:4])


def one_hot_line_end(rootname, family="last"):
    """the family's one-hot line from a root: (plies below the root at which the game ends, result, the last
    position, the placements of the positions before the root, of those on the line)"""
    fen, hist = root(rootname)
    g = O.Game(None if fen is None else O.from_fen(fen))
    before, after = [], []
    for a in hist:
        before.append(placement(g.position))
        assert g.play_index(int(a)) == 0
    ev = S.ref_evaluator(family)
    ply = 0
    while True:
        after.append(placement(g.position))
        idx = S.distinct(O.legal_indices(g.position))
        row = ev(g.position)[0]
        res = g.play_index(idx[int(np.argmax(row[idx]))])
        ply += 1
        if res != 0:
            return ply, res, g.position, before, after


@pytest.mark.parametrize("rootname", ["start", "lastline"])
def test_in_tree_repetition(rootname):
    """`last` sends every simulation down one line that ends in a third repetition: no other draw rule is
    due there, and the leaf is >= 6 plies below the root.  From the root five plies down that line the count
    spans the history before the root and the tree path."""
    r = step_refs("last")[("start", "lastline").index(rootname)]
    ply, res, pos, before, after = one_hot_line_end(rootname)
    line(r, "in-tree repetition")
    print("    the line ends %d plies below the root, halfmove clock %d, fullmove %d" % (ply, pos.halfmoves, pos.fullmoves))
    assert res == 1 and pos.halfmoves < 100 and pos.fullmoves < 200
    assert len(O.legal_indices(pos)) > 0 and not O.lib().ref_insufficient_material(pos)    # so: by repetition
    assert ply >= 6
    key = placement(pos)
    if rootname == "start":
        assert after.count(key) == 2 and before.count(key) == 0          # every repeated position on the tree path
    else:
        assert before.count(key) == 1 and after.count(key) == 1          # history and tree path together
    # the search went there: the node above the leaf, one expansion found the draw, the rest re-selected it
    assert r.depth == ply - 1 and r.counts["new_terminal"] == 1 and r.counts["known_terminal"] == r.sims - ply
    assert int(r.visits.max()) == r.sims


@pytest.mark.parametrize("name", ["uniform", "zeros64"])
def test_ties(name):
    r = step_refs(name)[0]
    line(r, "ties")
    assert r.root == "start" and r.sims == 64
    assert r.tally.ties >= 50
    assert r.tally.deep_ties >= 1                                      # below the root too
    line(step_refs(name)[1], "ties, game 1")


@pytest.mark.parametrize("name", ["zeros200", "nanmix200"])
def test_wide_nodes(name):
    r = step_refs(name)[0]
    line(r, "wide nodes")
    assert r.root == "wide" and r.sims == 200
    assert r.wide >= 20
    assert r.tally.wide_ties >= 1 or name != "zeros200"                # exact ties on the > 64-edge path
    line(step_refs(name)[1], "wide nodes, game 1")


def test_non_finite():
    r = step_refs("nanmix64")[0]
    line(r, "non-finite")
    assert r.root == "start" and int(r.visits.sum()) == r.sims == 64
    idx, row, _ = r.log[int(O.fen_key(O.startpos()))]
    nan_edges = [i for i in idx if np.isnan(row[i])]
    assert len(nan_edges) >= 1 and all(r.visits[i] == 0 for i in nan_edges)    # a NaN prior never wins
    assert r.tally.inf_taken >= 1
    assert any(np.isnan(v) for _, _, v in r.log.values())                      # NaN values were backed up
    for g, r in enumerate(step_refs("nanmix64")[1:], 1):
        line(r, "non-finite, game %d" % g)


def test_tree_reuse_on_a_chain():
    """every re-root of game 0 keeps a chain of >= 129 nodes: three 64-node chunks, each kept node's parent
    the node before it"""
    recs, _ = reuse_refs("hashed")
    for g, plies in enumerate(recs):
        print("reuse hashed game %d: (depth, carried, kept, result) %s"
              % (g, [(p["depth"], p["carried"], p["kept"], p["result"]) for p in plies]))
    assert len(recs[0]) == REUSE_PLIES
    for rec in recs[0][1:]:
        assert rec["kept"] >= 129 and rec["kept"] == rec["carried"] + 1


@pytest.mark.parametrize("family", ["nanmix", "zeros"])
def test_tree_reuse_keeps_part_of_the_tree(family):
    recs, tally = reuse_refs(family)
    for g, plies in enumerate(recs):
        print("reuse %s game %d: (depth, carried, kept, result) %s; ties %d fallback %d"
              % (family, g, [(p["depth"], p["carried"], p["kept"], p["result"]) for p in plies], tally.ties,
                 tally.fallback))
    assert len(recs[0]) == REUSE_PLIES
    for rec in recs[0][1:]:
        assert 65 <= rec["kept"] < REUSE_SIMS


def test_leaf_parallel_small_cases():
    for name in sorted(LEAF_CASES):
        for r in leaf_refs(name):
            line(r, name)
            assert int(r.visits.sum()) == r.sims
    assert all(r.tally.fallback == r.tally.selections for r in leaf_refs("allnan_k4"))    # always the first edge
    assert all(r.shared > 0 for name in LEAF_CASES if name[:-3] in ("nanmix", "allnan") for r in leaf_refs(name))


# ------------------------------------------------------------------ the references against each other
@pytest.mark.parametrize("name,noise", [(n, False) for n in STEP_CASES if n != "allnan"] + [(n, True) for n in NOISE_CASES])
def test_restatement_equals_the_c_oracle(name, noise):
    """K = 1, reuse off: leafpar_ref.search == O.search_game on visits, improved policy (as uint32) and depth.
    The C oracle aborts where nothing beats -inf (it keeps index 0, an illegal move), so a search goes to it
    only if the restatement never met such a node (RESTATEMENT_ONLY names the others)."""
    compared = 0
    for r in step_refs(name, noise):
        if r.tally.fallback:
            assert (name, r.root) in RESTATEMENT_ONLY, (name, r.root, r.tally.fallback)
            continue
        compared += 1
        cfg = O.make_cfg(sims=r.sims, noise=noise, seed=SEED, eval_kind=2)
        rv, ri, rd, evals = O.search_game(cfg, list(r.hist), noise=noise, noise_key=r.key or 0,
                                          replay=S.replay_of(r.log), start=r.start)
        assert np.array_equal(rv, r.visits), (name, r.root)
        assert np.array_equal(ri.view(np.uint32), r.improved.view(np.uint32)), (name, r.root)
        assert rd == r.depth, (name, r.root)
        if noise:
            line(r, "with noise")
    assert compared == sum(1 for r in step_refs(name, noise) if (name, r.root) not in RESTATEMENT_ONLY)


def test_allnan_takes_the_first_edge():
    """the restatement under allnan: every selection falls back to the first edge, so the tree is the line
    of first moves"""
    for r in step_refs("allnan"):
        line(r, "all NaN")
        assert r.tally.fallback == r.tally.selections and int(r.visits.sum()) == r.sims
        idx = S.distinct(O.legal_indices(r.start if r.start is not None else O.startpos()))
        assert r.visits[idx[0]] == r.sims


def test_selfplay_with_reuse_carries_visits():
    """the capped self-play restatement of test_gpu_sharp_search: 40 plies, every root topped up to 16 visits,
    visits carried; under `hashed` one move holds every visit of some roots"""
    for family in ("hashed", "zeros", "uniform"):
        game = reuse_selfplay_ref(family, 0, 5, 16, 40)
        assert all(int(rec["visits"].sum()) == 16 for rec in game)
        assert sum(rec["carried"] for rec in game) > 0
        one = sum(1 for rec in game if rec["visits"].max() == 16)
        print("selfplay with reuse, %s: %d plies, result %d, %d roots with one move visited" % (family, len(game), game[-1]["result"], one))
        assert one >= 1 or family != "hashed"
