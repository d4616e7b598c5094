"""Leaf-parallel search (az_search_cfg.leaves) restated in numpy f32 over the oracle's rules:
the yardstick of tests/test_gpu_leafpar.py.  TEST INFRASTRUCTURE ONLY.

A move's simulations run in waves.  One wave of k leaves: (1) select k leaves in order on the tree as it
stands, leaf j seeing, at every level, each earlier leaf of the wave through an edge as one more visit
that lost there (n = N + c, w = W - c, sqrt(nsum + c(node) + 1)); (2) classify each leaf by its last edge:
terminal, shared (an unexpanded edge that an earlier leaf of the wave ended on), or new; (3) expand the new
leaves in order, one evaluation each; (4) back all k up in order along their own paths.  With every wave of
size 1 this is the oracle's search (O.search_game), bit for bit."""
import ctypes

import numpy as np

import oracle as O

F = np.float32
DRAW, WIN = "draw", "win"          # an edge's child once the move is known to end the game


class Node:
    def __init__(self, game, policy):
        self.game = game                                                          # the GameState at this node
        idx = O.legal_indices(game.position)
        self.idx = np.array(list(dict.fromkeys(int(i) for i in idx)), np.int64)   # distinct, first appearance
        self.all_idx = idx                                                        # with under-promotion duplicates
        self.P = np.asarray(policy, F)[self.idx].copy()
        self.N = np.zeros(len(self.idx), np.int64)
        self.W = np.zeros(len(self.idx), F)
        self.child = [None] * len(self.idx)
        self.depth = 0


def clone_game(game):
    """GameState::clone: the position and its repetition multiset"""
    g = O.Game.__new__(O.Game)
    g._g = O.RefGame()
    O.lib().ref_game_clone(ctypes.byref(g._g), ctypes.byref(game._g))
    return g


def pick(node, c_edge, c_puct):
    """the edge of `node` the selection takes: first maximum of q + u, strict >, NaN never wins"""
    c = np.asarray(c_edge, np.int64)
    n = node.N + c
    w = node.W - c.astype(F)
    sq = np.sqrt(F(int(node.N.sum()) + int(c.sum()) + 1))
    nf = n.astype(F)
    u = F(c_puct) * node.P * sq / (F(1.0) + nf)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(n > 0, w / np.where(n > 0, nf, F(1.0)), F(0.0)).astype(F)
    v = q + u
    best, bpos = F(-np.inf), 0
    for e in range(len(v)):
        if v[e] > best:
            best, bpos = v[e], e
    return bpos


def search(start, history, waves, evaluator, noise_key=None, c_puct=3.0, alpha=0.3, eps=0.25, counts=None):
    """start: a RefPos or None (the startpos); history: move indices played from it to the root;
    waves: a list of wave sizes, or a tuple (sims, K) = waves of min(K, sims left);
    evaluator(RefPos) -> (policy [4096], value); noise_key: None = no root noise, else the Dirichlet
    stream key (O.lib().ref_stream_key(seed, game, ply, 0)).
    counts: a dict that receives how the simulations' leaves ended: "new_terminal" (the expansion found the
    game over: the engine's terminal_leaves), "known_terminal" (the selection ended on an edge already known
    to end the game: in none of the engine's counters), "shared_terminal" (shared leaves whose source's
    expansion found the game over; they are among the shared ones).
    -> visits [4096] f32, improved [4096] f32, depth, shared leaves, evaluations (the root's not counted)"""
    if isinstance(waves, tuple):
        sims, K = waves
        waves = [min(K, sims - i) for i in range(0, sims, K)]
    game = O.Game(start)
    for a in history:
        assert game.play_index(int(a)) == 0
    policy = np.array(evaluator(game.position)[0], F)
    root = Node(game, policy)
    if noise_key is not None and len(root.all_idx) >= 2:          # tree.rs:272-289, over the duplicates too
        eta = O.dirichlet(alpha, len(root.all_idx), noise_key)
        policy = policy * (F(1.0) - F(eps))
        for k, i in enumerate(root.all_idx):
            policy[i] = policy[i] + F(eps) * eta[k]
        root.P = policy[root.idx].copy()
    shared = evals = depth = 0
    tally = dict(new_terminal=0, known_terminal=0, shared_terminal=0)
    for k in waves:
        paths = []                                                # per leaf: [(node, edge)] from the root
        for j in range(k):
            node, path = root, []
            while True:
                L = len(path)
                c = [sum(1 for p in paths if len(p) > L and p[L][0] is node and p[L][1] == e)
                     for e in range(len(node.idx))]
                e = pick(node, c, c_puct)
                path.append((node, e))
                if not isinstance(node.child[e], Node):
                    break
                node = node.child[e]
            paths.append(path)
        kinds, values, src = [], [None] * k, [None] * k           # select is done: classify, then expand
        for j, path in enumerate(paths):
            node, e = path[-1]
            if node.child[e] in (DRAW, WIN):
                kinds.append("terminal")
                tally["known_terminal"] += 1
                values[j] = F(0.0) if node.child[e] == DRAW else F(-1.0)
                continue
            first = [i for i in range(j) if paths[i][-1][0] is node and paths[i][-1][1] == e]
            if first:
                kinds.append("shared")
                src[j] = first[0]
                shared += 1
            else:
                kinds.append("new")
        for j, path in enumerate(paths):
            if kinds[j] != "new":
                continue
            node, e = path[-1]
            g = clone_game(node.game)
            r = g.play_index(int(node.idx[e]))
            if r == 0:
                pol, val = evaluator(g.position)
                evals += 1
                ch = Node(g, pol)
                ch.depth = node.depth + 1
                depth = max(depth, ch.depth)
                node.child[e] = ch
                values[j] = F(val)
            else:
                assert r in (1, 2, 3), r
                node.child[e] = DRAW if r == 1 else WIN
                values[j] = F(0.0) if r == 1 else F(-1.0)
                tally["new_terminal"] += 1
                tally["shared_terminal"] += sum(1 for i in range(j + 1, k) if src[i] == j)
        for j, path in enumerate(paths):
            v = values[j] if src[j] is None else values[src[j]]
            n = len(path)
            for lv, (node, e) in enumerate(path):
                node.W[e] = node.W[e] + (v if (n - 1 - lv) & 1 else -v)
                node.N[e] += 1
    if counts is not None:
        counts.update(tally)
    visits = np.zeros(4096, F)
    visits[root.idx] = root.N.astype(F)
    with np.errstate(invalid="ignore"):
        improved = visits / visits.sum(dtype=F)
    return visits, improved.astype(F), depth, shared, evals
