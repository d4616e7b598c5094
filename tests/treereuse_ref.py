"""Tree reuse (az_search_set_tree_reuse) restated in numpy f32 over the oracle's rules: the
yardstick of tests/test_gpu_treereuse.py.  TEST INFRASTRUCTURE ONLY.

The definition.  (1) Re-root: the Node of the played move becomes the root as it stands -- its priors,
scores, visits and children, every node below it; everything else is dropped; depths are rebased so the new
root's is 0, and the search depth starts at the largest rebased depth kept.  With noise the Dirichlet noise
of the stream (seed, game, ply, 0) goes onto the root's priors; visits and scores stay.  (2) A move's
search: the reference's simulation loop (tree.rs:117-144; leafpar_ref's pick with no virtual loss) on that
tree while the root's visits sum to less than `sims`, so sims - carried >= 1 simulations; the improved
policy and the move choice come from the root's visits.  (3) Fresh roots carry nothing: with nothing
carried, a move is the oracle's search (O.search_game), bit for bit."""
import ctypes

import numpy as np

import oracle as O
from leafpar_ref import DRAW, WIN, Node, clone_game, pick

F = np.float32
NUM_FULLMOVES = 200                 # parameters.rs: the 200-fullmove draw, and the final value's decay


def stream_key(seed, game, ply, purpose=0):
    return O.lib().ref_stream_key(seed, game, ply, purpose)


def uniform01(key):
    """the first draw of the stream `key` (training.rs:318-321's thread_rng stand-in)"""
    fn = O.lib().ref_uniform01
    fn.argtypes = [ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64)]
    fn.restype = ctypes.c_float
    ctr = ctypes.c_uint64(0)
    return F(fn(key, ctypes.byref(ctr)))


def subtree(node):
    """every Node of the subtree, the root first"""
    out, stack = [], [node]
    while stack:
        n = stack.pop()
        out.append(n)
        stack += [c for c in n.child if isinstance(c, Node)]
    return out


class Search:
    """One game's search carried across plies.  evaluator(RefPos) -> (policy [4096], value)."""

    def __init__(self, history=(), evaluator=O.synth_eval, sims=32, noise_key=None, start=None, c_puct=3.0,
                 alpha=0.3, eps=0.25):
        self.evaluator, self.sims, self.c_puct, self.alpha, self.eps = evaluator, sims, c_puct, alpha, eps
        self.game = O.Game(start)
        for a in history:
            assert self.game.play_index(int(a)) == 0
        self.fresh(noise_key)

    def fresh(self, noise_key=None):
        """a root that carries nothing (set_roots, a restarted slot, adopt): MCTree::new on the game so far"""
        self.root = Node(clone_game(self.game), np.array(self.evaluator(self.game.position)[0], F))
        self.depth = 0
        self.noise(noise_key)

    def noise(self, noise_key):
        """tree.rs:272-289 on the root's priors as they stand, over the under-promotion duplicates too"""
        root = self.root
        if noise_key is None or len(root.all_idx) < 2:
            return
        eta = O.dirichlet(self.alpha, len(root.all_idx), noise_key)
        policy = np.zeros(4096, F)
        policy[root.idx] = root.P
        policy = policy * (F(1.0) - F(self.eps))
        for k, i in enumerate(root.all_idx):
            policy[i] = policy[i] + F(self.eps) * eta[k]
        root.P = policy[root.idx].copy()

    def run(self):
        """one move's search -> dict(visits [4096] f32, improved [4096] f32, depth, carried (the root's visits
        before it), kept (nodes before it), sims (simulations run), evals, new_terminal (expansions that found
        the game over), known_terminal (leaves selected onto an edge already known to end the game))"""
        root = self.root
        out = dict(carried=int(root.N.sum()), kept=len(subtree(root)), sims=0, evals=0, new_terminal=0,
                   known_terminal=0)
        zeros = {}
        while int(root.N.sum()) < self.sims:
            node, path = root, []
            while True:
                n = len(node.idx)
                e = pick(node, zeros.setdefault(n, np.zeros(n, np.int64)), self.c_puct)
                path.append((node, e))
                if not isinstance(node.child[e], Node):
                    break
                node = node.child[e]
            if node.child[e] in (DRAW, WIN):
                out["known_terminal"] += 1
                v = F(0.0) if node.child[e] == DRAW else F(-1.0)
            else:
                g = clone_game(node.game)
                r = g.play_index(int(node.idx[e]))
                if r == 0:
                    pol, val = self.evaluator(g.position)
                    out["evals"] += 1
                    ch = Node(g, pol)
                    ch.depth = node.depth + 1
                    self.depth = max(self.depth, ch.depth)
                    node.child[e] = ch
                    v = F(val)
                else:
                    assert r in (1, 2, 3), r
                    node.child[e] = DRAW if r == 1 else WIN
                    v = F(0.0) if r == 1 else F(-1.0)
                    out["new_terminal"] += 1
            n = len(path)
            for lv, (nd, ed) in enumerate(path):
                nd.W[ed] = nd.W[ed] + (v if (n - 1 - lv) & 1 else -v)
                nd.N[ed] += 1
            out["sims"] += 1
        visits = np.zeros(4096, F)
        visits[root.idx] = root.N.astype(F)
        out.update(visits=visits, improved=(visits / visits.sum(dtype=F)).astype(F), depth=self.depth)
        return out

    def last_max(self):
        """training.rs:310-317: the LAST maximum of the visits in index order"""
        root = self.root
        best = max(zip(root.N.tolist(), root.idx.tolist()))
        return int(best[1])

    def weighted(self, key):
        """training.rs:318-321: WeightedIndex over visits / sum in index order, f32 cumulative sums"""
        root = self.root
        order = np.argsort(root.idx)
        totf = F(int(root.N.sum()))
        w = [(int(root.idx[o]), F(int(root.N[o])) / totf) for o in order if root.N[o]]
        total = F(0.0)
        for _, x in w:
            total = total + x
        x = uniform01(key) * total
        if not x < total:
            x = np.nextafter(total, F(0.0))
        cw = F(0.0)
        for i, p in w:
            cw = cw + p
            if cw > x:
                return i
        return w[-1][0]

    def advance(self, action, noise_key=None):
        """play `action` and re-root on its Node, keeping the subtree -> the move's result (0: the game goes on)"""
        root = self.root
        e = int(np.nonzero(root.idx == int(action))[0][0])
        r = self.game.play_index(int(action))
        if r != 0:
            assert root.child[e] == (DRAW if r == 1 else WIN), (r, root.child[e])
            self.root = None
            return r
        ch = root.child[e]
        assert isinstance(ch, Node)
        d0 = ch.depth
        nodes = subtree(ch)
        for n in nodes:
            n.depth -= d0
        self.depth = max(n.depth for n in nodes)
        self.root = ch
        self.noise(noise_key)
        return 0


def stepwise(history, game, plies, sims, seed=None, evaluator=O.synth_eval):
    """The stepwise API's run() + advance(last maximum) for `plies` plies from `history`; seed = None: no
    noise, else the noise of (seed, game, ply, 0) at every root -> [Search.run()'s dict + action, result (of
    playing it: 0 = the game goes on) and what that re-root kept (next_carried, next_kept) per ply].  A game that ends is searched no further (the engine leaves an
    inactive game untouched): the list ends with the ply whose result is not 0."""
    key = (lambda p: stream_key(seed, game, p)) if seed is not None else (lambda p: None)
    s = Search(history, evaluator, sims, key(len(history)))
    out = []
    for p in range(plies):
        rec = s.run()
        rec["action"] = s.last_max()
        rec["result"] = s.advance(rec["action"], key(len(history) + p + 1))
        if rec["result"] == 0:                                # what the re-root kept (az_search_reuse_stats)
            rec["next_carried"], rec["next_kept"] = int(s.root.N.sum()), len(subtree(s.root))
        out.append(rec)
        if rec["result"] != 0:
            break
    return out


def selfplay_game(game, seed, sims, evaluator=O.synth_eval, noise=True, temp_moves=15):
    """training.rs:294-338 with tree reuse: game `game` from the startpos to its end -> [per ply: Search.run()'s
    dict + action, result, final_value]"""
    key = (lambda p: stream_key(seed, game, p)) if noise else (lambda p: None)
    s = Search((), evaluator, sims, key(0))
    out, ply = [], 0
    while True:
        rec = s.run()
        pos = s.game.position
        rec["turn"] = F(1.0) if pos.turn == 0 else F(-1.0)
        rec["action"] = s.last_max() if pos.fullmoves >= temp_moves else s.weighted(stream_key(seed, game, ply, 1))
        out.append(rec)
        ply += 1
        r = s.advance(rec["action"], key(ply))
        if r != 0:
            break
    result = F(0.0) if r == 1 else (F(1.0) if r == 2 else F(-1.0))
    decay = F(1.0) - (F(s.game.position.fullmoves) / (F(2.0) * F(NUM_FULLMOVES)))
    for rec in out:
        rec["result"] = r
        rec["final_value"] = F(rec["turn"] * (result * decay))
    return out
