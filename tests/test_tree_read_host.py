"""Whole-tree read-out (az_search_read_tree / az_search_read_pv) on the host: the ABI's
symbols, records and NULL-handle failures, azchess.tree_views on hand-made arrays, and the cases of
tests/test_gpu_tree_read.py -- their roots, the restatement's trees (tests/treereuse_ref.py) flattened by
path, and the conditions those cases rest on, stated from the restatement alone.  No GPU."""
import ctypes as C
import functools
import os

import numpy as np

import azchess as A
import azchess._lib as L
import oracle as O
import treereuse_ref as R
from azchess.tree import TreeView, tree_views
from leafpar_ref import DRAW, WIN, Node

F = np.float32
SEED = 29
SIMS = 32
START_FEN = "rnbqkbnr/pppppppp/8/8/8/8/PPPPPPPP/RNBQKBNR w KQkq - 0 1"
# (fen or None = the startpos, history): a move from mate, a capture away from bare kings, a pawn on the
# seventh rank, and three roots of the opening
def opening(plies):
    """a legal history from the startpos: ply i plays entry (7 i + 3) mod n of its legal moves"""
    p, h = A.Position.startpos(), []
    for i in range(plies):
        idx = p.legal_indices()
        h.append(int(idx[(7 * i + 3) % len(idx)]))
        p = p.play(h[-1])
    return h


ROOTS = [
    ("7k/8/6K1/8/8/8/Q7/8 w - - 0 1", []),
    ("8/8/8/8/8/8/1p6/K2k4 w - - 0 1", []),
    ("4k3/1P6/8/8/8/8/6p1/4K3 w - - 0 1", []),
    (None, []),
    (None, opening(1)),
    (None, opening(5)),
]
DEEP_SIMS = 512                      # case 2: one game from the startpos, several 64-node chunks


def start_of(fen):
    return None if fen is None else O.from_fen(fen)


def host_position(fen, moves):
    """the engine's own host rules: az_pos of the root's start with `moves` played"""
    p = A.Position.startpos() if fen is None else A.Position.from_fen(fen)
    for a in moves:
        p = p.play(int(a))
    return p


def noise_key(noise, game, ply, seed=SEED):
    return R.stream_key(seed, game, ply) if noise else None


# ------------------------------------------------------------------ trees by path
def flatten_ref(root):
    """the restatement's tree -> {path (move indices from the root): record}; a record holds the edge
    rows in edge order as bit patterns, each edge's child kind, depth, nsum and the node's FEN"""
    out, stack = {}, [((), root)]
    while stack:
        path, n = stack.pop()
        kinds = []
        for e, c in enumerate(n.child):
            if isinstance(c, Node):
                kinds.append("node")
                stack.append((path + (int(n.idx[e]),), c))
            else:
                kinds.append({None: "none", DRAW: "draw", WIN: "win"}[c])
        dup = [int(i) for i in n.all_idx]
        out[path] = dict(index=[int(i) for i in n.idx], prior=n.P.astype(F).view(np.uint32).tolist(),
                         score=n.W.astype(F).view(np.uint32).tolist(), visits=[int(v) for v in n.N], kinds=kinds,
                         promo=[dup.count(int(i)) == 4 for i in n.idx], depth=int(n.depth), nsum=int(n.N.sum()),
                         fen=O.to_fen(n.game.position))
    return out


KIND = {L.TREE_UNEXPANDED: "none", L.TREE_DRAW: "draw", L.TREE_WIN: "win", L.TREE_CUT: "cut"}


def flatten_view(view, with_state=True):
    """an exported tree -> the same mapping, plus each node's ordinal, parent ordinal and state bytes"""
    out, stack = {}, [((), view)]
    while stack:
        path, v = stack.pop()
        e = v.edges
        rec = dict(index=e["index"].tolist(), prior=e["prior"].view(np.uint32).tolist(),
                   score=e["score"].view(np.uint32).tolist(), visits=e["visits"].tolist(),
                   kinds=["node" if c >= 0 else KIND[int(c)] for c in e["child"]],
                   promo=[bool(f & 1) for f in e["flags"]], depth=v.depth, nsum=v.nsum, ordinal=v.ordinal,
                   parent=int(v.record["parent"]), parent_edge=int(v.record["parent_edge"]))
        if with_state:
            st = v.state
            rec["fen"], rec["state"] = st.fen(), st.raw()
        out[path] = rec
        for i, ch in v.nodes.items():
            stack.append((path + (i,), ch))
    return out


COMPARED = ("index", "prior", "score", "visits", "kinds", "promo", "depth", "nsum", "fen")


def assert_same_tree(view, ref_root, fen, history, what=""):
    """every node reached by a path: equal priors, scores, visits (bit patterns), edge order, child kinds,
    depth, nsum and state; equal node and edge counts; parents precede children"""
    got, ref = flatten_view(view), flatten_ref(ref_root)
    assert set(got) == set(ref), (what, sorted(set(got) ^ set(ref))[:5])
    for path in sorted(ref, key=len):
        g, r = got[path], ref[path]
        for k in COMPARED:
            assert g[k] == r[k], (what, path, k, g[k], r[k])
        assert g["state"] == host_position(fen, list(history) + list(path)).raw(), (what, path)
    assert len(view._nodes) == len(ref) and len(view._edges) == sum(len(r["index"]) for r in ref.values()), what
    assert_well_formed(view, what)


def assert_well_formed(view, what=""):
    """node 0 is the root, parents precede children, every node's parent_edge leads to it, the edge ranges
    tile the game's edges in node order"""
    n, e = view._nodes, view._edges
    assert n["parent"][0] == -1 and n["parent_edge"][0] == -1 and n["depth"][0] == 0, what
    at = 0
    for i in range(len(n)):
        assert n["edge_begin"][i] == at, (what, i)
        at += int(n["nedges"][i])
        if i:
            p = int(n["parent"][i])
            assert 0 <= p < i and n["depth"][i] == n["depth"][p] + 1, (what, i)
            assert e["child"][n["edge_begin"][p] + n["parent_edge"][i]] == i, (what, i)
    assert at == len(e), what
    kids = e["child"][e["child"] >= 0]
    assert sorted(kids.tolist()) == list(range(1, len(n))), what


def pv_of(index, visits, score, child_of):
    """the stated rule on one tree: from the root the most visited edge, ties to the larger index, down while
    it has a child node; stops before a 0-visit edge.  index / visits / score: node -> rows; child_of(node,
    e) -> the child node or None.  -> (moves, q of the first move as f32, its visits)"""
    moves, q, vis, node = [], F(0.0), 0, "root"
    while node is not None:
        iv = list(zip(visits(node), index(node)))
        if not iv or max(iv)[0] == 0:
            break
        e = iv.index(max(iv))
        if not moves:
            q, vis = F(score(node)[e]) / F(iv[e][0]), iv[e][0]
        moves.append(iv[e][1])
        node = child_of(node, e)
    return moves, q, vis


def pv_ref(root, cap):
    get = lambda n: root if isinstance(n, str) else n
    m, q, v = pv_of(lambda n: [int(i) for i in get(n).idx], lambda n: [int(x) for x in get(n).N], lambda n: get(n).W,
                    lambda n, e: get(n).child[e] if isinstance(get(n).child[e], Node) else None)
    return (m[:cap], q, v) if cap else ([], F(0.0), 0)


def pv_view(view, cap):
    get = lambda n: view if isinstance(n, str) else n
    m, q, v = pv_of(lambda n: get(n).edges["index"].tolist(), lambda n: get(n).edges["visits"].tolist(),
                    lambda n: get(n).edges["score"],
                    lambda n, e: (TreeView(view._nodes, view._edges, view._states, get(n).edges["child"][e])
                                  if get(n).edges["child"][e] >= 0 else None))
    return (m[:cap], q, v) if cap else ([], F(0.0), 0)


# ------------------------------------------------------------------ the restatement's trees, computed once
@functools.lru_cache(maxsize=None)
def case_search(k, noise, sims=SIMS):
    """root k's restatement after `sims` simulations (tree reuse's restatement with nothing carried is the
    oracle's search, tests/test_treereuse_host.py)"""
    fen, h = ROOTS[k]
    s = R.Search(h, O.synth_eval, sims, noise_key(noise, k, len(h)), start=start_of(fen))
    s.run()
    return s


@functools.lru_cache(maxsize=None)
def deep_search():
    s = R.Search((), O.synth_eval, DEEP_SIMS, None)
    s.run()
    return s


def test_case_conditions():
    """what the GPU cases rest on: within 32 simulations a DRAW edge, a WIN edge and a promotion edge with a
    child node all appear, with and without noise; some root's two most visited edges tie; the 512-simulation
    tree spans several 64-node chunks"""
    ties = 0
    for noise in (False, True):
        flat = [flatten_ref(case_search(k, noise).root) for k in range(len(ROOTS))]
        kinds = lambda f: {k for r in f.values() for k in r["kinds"]}
        assert "win" in kinds(flat[0]) and "draw" in kinds(flat[1]), noise
        assert any(p and k == "node" for r in flat[2].values() for p, k in zip(r["promo"], r["kinds"])), noise
        for f in flat:
            top = sorted(f[()]["visits"])[-2:]
            ties += len(top) == 2 and top[0] == top[1] > 0
            assert sum(f[()]["visits"]) == SIMS
    assert ties >= 1
    assert len(flatten_ref(deep_search().root)) > 4 * 64


def test_pv_rule_on_the_restatement():
    s = case_search(0, False)                                  # the mate in one is found and ends the PV
    m, q, v = pv_ref(s.root, 64)
    assert len(m) == 1 and s.root.child[int(np.nonzero(s.root.idx == m[0])[0][0])] == WIN and q == F(1.0)
    assert pv_ref(s.root, 0) == ([], F(0.0), 0)


# ------------------------------------------------------------------ the ABI
def test_symbols_records_and_markers():
    for name in ("az_search_read_tree", "az_search_read_pv"):
        assert hasattr(L.lib, name), name
    assert C.sizeof(L.AzTreeNode) == 24 and C.sizeof(L.AzTreeEdge) == 24
    assert L.TREE_NODE_DTYPE.itemsize == 24 and L.TREE_EDGE_DTYPE.itemsize == 24
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "az.h")).read()
    for name, val in (("AZ_TREE_UNEXPANDED", L.TREE_UNEXPANDED), ("AZ_TREE_DRAW", L.TREE_DRAW),
                      ("AZ_TREE_WIN", L.TREE_WIN), ("AZ_TREE_CUT", L.TREE_CUT)):
        assert "%s = %d" % (name, val) in hdr, name
    assert (L.TREE_UNEXPANDED, L.TREE_DRAW, L.TREE_WIN, L.TREE_CUT) == (-1, -2, -3, -4)


def test_null_handles_fail_cleanly():
    off = (C.c_int64 * 2)(7, 7)
    rc = L.lib.az_search_read_tree(None, None, 0, 0, -1, off, off, None, 0, None, 0, None)
    assert rc < 0 and b"null" in L.lib.az_last_error() and list(off) == [7, 7]
    mv = (C.c_int32 * 4)(9, 9, 9, 9)
    rc = L.lib.az_search_read_pv(None, mv, 4, None, None, None)
    assert rc < 0 and b"null" in L.lib.az_last_error() and list(mv) == [9, 9, 9, 9]


# ------------------------------------------------------------------ tree_views on hand-made arrays
def hand_made():
    """two games.  Game 0: a root with 4 edges -- a promotion edge (index 3529) that leads to node 1, a draw
    edge, a cut edge and an unexpanded one; node 1 has one winning edge.  Game 1: a lone root, 1 edge."""
    nodes = np.zeros(3, L.TREE_NODE_DTYPE)
    edges = np.zeros(6, L.TREE_EDGE_DTYPE)
    nodes[0] = (-1, -1, 0, 4, 0, 9)
    nodes[1] = (0, 0, 4, 1, 1, 2)
    nodes[2] = (-1, -1, 0, 1, 0, 0)
    edges[0] = (0.5, 1.5, 4, 3529, 1, 1)
    edges[1] = (0.25, 0.0, 2, 17, L.TREE_DRAW, 0)
    edges[2] = (0.125, -1.0, 3, 4095, L.TREE_CUT, 0)
    edges[3] = (0.125, 0.0, 0, 0, L.TREE_UNEXPANDED, 0)
    edges[4] = (1.0, 2.0, 2, 100, L.TREE_WIN, 0)
    edges[5] = (1.0, 0.0, 0, 7, L.TREE_UNEXPANDED, 0)
    states = np.zeros(3, L.POS_DTYPE)
    states.view(np.uint8).reshape(3, 80)[:] = np.frombuffer(A.Position.startpos().raw(), np.uint8)
    states["fullmoves"] = [1, 2, 3]
    return np.array([0, 2, 3]), np.array([0, 5, 6]), nodes, edges, states


def test_tree_views_navigate_hand_made_arrays():
    noff, eoff, nodes, edges, states = hand_made()
    views = tree_views(noff, eoff, nodes, edges, states)
    assert len(views) == 2
    root, lone = views
    # the promotion edge stands for four entries of `moves`
    assert root.moves.tolist() == [3529, 3529, 3529, 3529, 17, 4095, 0]
    for name, field in (("policy", "prior"), ("visits", "visits"), ("scores", "score")):
        row = getattr(root, name)
        assert row.dtype == np.float32 and row.shape == (4096,)
        want = np.zeros(4096, F)
        want[[3529, 17, 4095, 0]] = edges[field][:4]
        assert np.array_equal(row, want), name
    assert list(root.nodes) == [3529] and root.terminal == {17: "draw"} and root.cut == [4095]
    assert (root.depth, root.nsum, root.max_subtree_depth()) == (0, 9, 1)
    child = root.nodes[3529]
    assert (child.ordinal, child.depth, child.nsum, child.max_subtree_depth()) == (1, 1, 2, 0)
    assert child.moves.tolist() == [100] and child.terminal == {100: "win"} and child.nodes == {} and child.cut == []
    assert child.scores[100] == F(2.0) and child.visits.sum() == F(2.0)
    assert (root.state.fullmoves, child.state.fullmoves, lone.state.fullmoves) == (1, 2, 3)
    # the second game's view is its own: ordinals and edges relative to its ranges
    assert lone.moves.tolist() == [7] and lone.nodes == {} and lone.max_subtree_depth() == 0 and lone.nsum == 0
    # without states the fields still read; the state does not
    bare = tree_views(noff, eoff, nodes, edges)[0]
    assert bare.nodes[3529].moves.tolist() == [100]
    try:
        bare.state
        assert False, "a view without states has no state"
    except ValueError:
        pass
    assert set(flatten_view(root)) == {(), (3529,)}
