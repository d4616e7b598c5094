"""tree.rs mirror: MCTree over the GPU-resident batched search (libaz az_search_*).

`MCTree` is one game's tree with the reference's method names; `BatchedSearch` runs G trees
in lockstep on one GPU (what the engine actually does for self-play).
"""
import ctypes as C

import numpy as np

from . import _lib as L
from .parameters import CACHE_CAPACITY, C_PUCT, DIRICHLET_ALPHA, DIRICHLET_EPSILON, NUM_SIMULATIONS, SEED, TEMPERATURE_ANNEALING


def make_cfg(games, sims=NUM_SIMULATIONS, c_puct=C_PUCT, dir_alpha=DIRICHLET_ALPHA, dir_eps=DIRICHLET_EPSILON,
             temp_moves=TEMPERATURE_ANNEALING, noise=True, seed=SEED, synthetic=False, continuous=False,
             record_evals=False, eval_log_cap=0, cache_capacity=CACHE_CAPACITY, callback=False, leaves=1):
    """leaves: leaf-parallel search, K leaves per game per simulation step (1..8; 1 = the reference's
    search).  K > 1 changes the results: see az_search_cfg.leaves."""
    kind = L.EVAL_CALLBACK if callback else (L.EVAL_SYNTHETIC if synthetic else L.EVAL_NET)
    return L.AzSearchCfg(games, sims, c_puct, dir_alpha, dir_eps, temp_moves, 1 if noise else 0, seed,
                         kind, 1 if continuous else 0, 1 if record_evals else 0, eval_log_cap, cache_capacity, leaves)


def _eval_trampoline(evaluator):
    """az_eval_fn around a Python process_batch-style callable (training.rs:380-422):
    evaluator(positions) -> (policy [n, 4096], value [n]); its rows are copied into the engine's
    staging buffers."""
    from .chess import Position

    def fn(_ctx, pos, n, pol, val):
        try:
            states = [Position(L.AzPos.from_buffer_copy(pos[i])) for i in range(n)]
            p, v = evaluator(states)
            np.ctypeslib.as_array(pol, shape=(n * 4096,))[:] = np.asarray(p, np.float32).reshape(n * 4096)
            np.ctypeslib.as_array(val, shape=(n,))[:] = np.asarray(v, np.float32).reshape(n)
            return 0
        except BaseException as e:              # nothing may unwind through the C frames, not even
            import traceback                    # KeyboardInterrupt / SystemExit (ctypes would swallow
            traceback.print_exc()               # them and report success over stale staging rows)
            if not isinstance(e, Exception):
                pending[0] = e
            return 1
    pending = [None]
    return L.EVAL_FN(fn), pending


class TreeView:
    """One node of an exported search tree (BatchedSearch.read_tree) with the reference's field names
    (MCTree, tree.rs:25-34): a light view over one game's numpy record arrays (L.TREE_NODE_DTYPE,
    L.TREE_EDGE_DTYPE, L.POS_DTYPE), rooted at node `ordinal`.  Nothing is copied until a field is read."""

    __slots__ = ("_nodes", "_edges", "_states", "ordinal")

    def __init__(self, nodes, edges, states=None, ordinal=0):
        self._nodes, self._edges, self._states, self.ordinal = nodes, edges, states, int(ordinal)

    @property
    def record(self):
        """the node's az_tree_node record"""
        return self._nodes[self.ordinal]

    @property
    def edges(self):
        """the node's az_tree_edge records, in the order the selection scans them"""
        r = self._nodes[self.ordinal]
        return self._edges[int(r["edge_begin"]):int(r["edge_begin"]) + int(r["nedges"])]

    @property
    def moves(self):
        """legal move indices in legal_moves() order of first appearance, a promotion's index four times
        (tree.rs:86-89)"""
        e = self.edges
        return np.repeat(e["index"], np.where(e["flags"] & L.TREE_EDGE_PROMO, 4, 1)).astype(np.int32)

    def _dense(self, field):
        e = self.edges
        out = np.zeros(L.ACTION_SPACE, np.float32)
        out[e["index"]] = e[field]
        return out

    @property
    def policy(self):
        """dense [4096] f32 priors (noised at a noised root)"""
        return self._dense("prior")

    @property
    def visits(self):
        return self._dense("visits")

    @property
    def scores(self):
        return self._dense("score")

    @property
    def nodes(self):
        """move index -> child TreeView, for the edges whose child node is in the export"""
        return {int(e["index"]): TreeView(self._nodes, self._edges, self._states, e["child"])
                for e in self.edges if e["child"] >= 0}

    @property
    def terminal(self):
        """move index -> "draw" / "win" for the moves known to end the game"""
        return {int(e["index"]): "draw" if e["child"] == L.TREE_DRAW else "win"
                for e in self.edges if e["child"] in (L.TREE_DRAW, L.TREE_WIN)}

    @property
    def cut(self):
        """move indices whose child node min_visits / max_depth left out of the export"""
        return [int(e["index"]) for e in self.edges if e["child"] == L.TREE_CUT]

    @property
    def state(self):
        """the node's Position (read_tree(states=True))"""
        if self._states is None:
            raise ValueError("the tree was read without states (read_tree(states=True))")
        from .chess import array_position
        return array_position(self._states, self.ordinal)

    @property
    def depth(self):
        return int(self._nodes[self.ordinal]["depth"])

    @property
    def nsum(self):
        """visits summed over the node's edges"""
        return int(self._nodes[self.ordinal]["nsum"])

    def max_subtree_depth(self):
        """the deepest exported node below this one, in plies from it (tree.rs:258-269)"""
        n = self._nodes
        below = np.zeros(len(n), bool)
        below[self.ordinal] = True
        for i in range(self.ordinal + 1, len(n)):        # parents precede their children
            below[i] = below[n["parent"][i]]
        return int(n["depth"][below].max()) - self.depth


def tree_views(node_off, edge_off, nodes, edges, states=None):
    """The root TreeView of every game of an az_search_read_tree export (CSR offsets and record arrays; a pure
    host function)."""
    out = []
    for k in range(len(node_off) - 1):
        n0, n1, e0, e1 = int(node_off[k]), int(node_off[k + 1]), int(edge_off[k]), int(edge_off[k + 1])
        out.append(TreeView(nodes[n0:n1], edges[e0:e1], None if states is None else states[n0:n1]))
    return out


class BatchedSearch:
    """G concurrent game trees on one device."""

    def __init__(self, model=None, games=1, device=0, evaluator=None, tree_reuse=False, **cfg):
        """model: an AlphaZero (AZ_EVAL_NET); evaluator: a caller-owned process_batch-style callable
        (AZ_EVAL_CALLBACK); neither: the synthetic evaluator the oracle shares.
        tree_reuse (opt-in; False: every re-root starts from an empty tree, the reference's traverse_new):
        advance() and the self-play driver keep the played move's subtree and a move's search tops the
        root up to `sims` visits (az_search_set_tree_reuse).  A different search from the reference's;
        not with leaves > 1."""
        synthetic = model is None and evaluator is None
        self.cfg = make_cfg(games, synthetic=synthetic, callback=evaluator is not None, **cfg)
        self.games = games
        self.model = model
        h = C.c_void_p()
        L.check(L.lib.az_search_create(model._h if model is not None else None, C.byref(self.cfg), device,
                                       C.byref(h)))
        self._h = h
        self._eval_fn, self._pending = None, [None]
        if evaluator is not None:
            self._eval_fn, self._pending = _eval_trampoline(evaluator)     # kept alive as long as the engine
            L.check(L.lib.az_search_set_evaluator(self._h, C.cast(self._eval_fn, C.c_void_p), None))
        if tree_reuse:
            self.set_tree_reuse(True)

    def set_tree_reuse(self, on):
        """az_search_set_tree_reuse: before the first set_roots() / SelfPlay.reset() only."""
        L.check(L.lib.az_search_set_tree_reuse(self._h, int(on)))

    @property
    def tree_reuse(self):
        """True if re-roots keep the played move's subtree."""
        on = C.c_int()
        L.check(L.lib.az_search_reuse_stats(self._h, C.byref(on), None, None, None))
        return bool(on.value)

    def reuse_stats(self):
        """{reroots, carried_visits, carried_nodes}: re-roots that kept a subtree, the visits their new
        roots held and the nodes kept, since creation or the last SelfPlay.reset()."""
        r, v, n = C.c_uint64(), C.c_uint64(), C.c_uint64()
        L.check(L.lib.az_search_reuse_stats(self._h, None, C.byref(r), C.byref(v), C.byref(n)))
        return {"reroots": r.value, "carried_visits": v.value, "carried_nodes": n.value}

    def __del__(self):
        try:
            L.lib.az_search_destroy(self._h)
        except Exception:
            pass

    def check(self, rc):
        """L.check for calls that may run the caller's evaluator: a KeyboardInterrupt / SystemExit
        raised inside it is re-raised here, after the C call has returned its error."""
        e, self._pending[0] = self._pending[0], None
        if e is not None:
            raise e
        return L.check(rc)

    def set_roots(self, histories, apply_noise=False, game_ids=None, noise_plies=None, start=None):
        """MCTree::new(eval(root), state, apply_noise) for each game; state = start + history
        (start: a list of G Positions, e.g. from FENs; None = the startpos)."""
        assert len(histories) == self.games
        off = np.zeros(self.games + 1, np.int32)
        for g, h in enumerate(histories):
            off[g + 1] = off[g] + len(h)
        flat = np.ascontiguousarray(np.concatenate([np.asarray(h, np.int32) for h in histories] + [np.zeros(1, np.int32)]))
        gid = np.arange(self.games, dtype=np.int32) if game_ids is None else np.asarray(game_ids, np.int32)
        plies = (off[1:] - off[:-1]).astype(np.int32) if noise_plies is None else np.asarray(noise_plies, np.int32)
        st = None
        if start is not None:
            assert len(start) == self.games
            st = (L.AzPos * self.games)()
            for g, p in enumerate(start):
                st[g] = p._p
        self.check(L.lib.az_search_set_roots_from(self._h, st, L.i32ptr(flat), L.i32ptr(off), L.i32ptr(gid),
                                               L.i32ptr(plies), 1 if apply_noise else 0))

    def run(self):
        """monte_carlo_tree_search for every game -> (improved [G,4096], visits [G,4096], depth [G])."""
        imp = np.zeros((self.games, 4096), np.float32)
        vis = np.zeros((self.games, 4096), np.uint32)
        dep = np.zeros(self.games, np.int32)
        self.check(L.lib.az_search_run(self._h, L.fptr(imp), L.u32ptr(vis), L.i32ptr(dep)))
        return imp, vis, dep

    def read_roots(self):
        """(improved [G,4096], visits [G,4096], depth [G]) of the current roots, no simulations run
        (the reference's public MCTree fields, tree.rs:25-34)."""
        imp = np.zeros((self.games, 4096), np.float32)
        vis = np.zeros((self.games, 4096), np.uint32)
        dep = np.zeros(self.games, np.int32)
        L.check(L.lib.az_search_read_roots(self._h, L.fptr(imp), L.u32ptr(vis), L.i32ptr(dep)))
        return imp, vis, dep

    def read_tree_arrays(self, games=None, min_visits=0, max_depth=None, states=False):
        """az_search_read_tree -> (node_off, edge_off, nodes, edges, states or None): the CSR export of the
        listed slots' trees (None: all), sized by a first call and filled by a second."""
        if games is None:
            gl, n = None, self.games
        else:
            gl = np.ascontiguousarray(games, np.int32)
            n = len(gl)
        gp = None if gl is None else L.i32ptr(gl)
        md = -1 if max_depth is None else int(max_depth)
        noff, eoff = np.zeros(n + 1, np.int64), np.zeros(n + 1, np.int64)
        i64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))
        L.check(L.lib.az_search_read_tree(self._h, gp, n, int(min_visits), md, i64(noff), i64(eoff), None, 0, None, 0,
                                          None))
        nodes = np.zeros(max(int(noff[n]), 1), L.TREE_NODE_DTYPE)
        edges = np.zeros(max(int(eoff[n]), 1), L.TREE_EDGE_DTYPE)
        pos = np.zeros(max(int(noff[n]), 1), L.POS_DTYPE) if states else None
        L.check(L.lib.az_search_read_tree(
            self._h, gp, n, int(min_visits), md, i64(noff), i64(eoff),
            nodes.ctypes.data_as(C.POINTER(L.AzTreeNode)), len(nodes), edges.ctypes.data_as(C.POINTER(L.AzTreeEdge)),
            len(edges), pos.ctypes.data_as(C.POINTER(L.AzPos)) if states else None))
        return noff, eoff, nodes[:int(noff[n])], edges[:int(eoff[n])], pos[:int(noff[n])] if states else None

    def read_tree(self, games=None, min_visits=0, max_depth=None, states=False):
        """The search trees of the listed slots (None: all) as they stand, read from the device: a list of
        root TreeViews with the reference's MCTree fields at every node.  A child node is exported only if
        its edge has visits >= min_visits and its depth is <= max_depth (None: no limit; 0: the roots alone);
        where that leaves an existing child out the move is listed in TreeView.cut.  states=True also
        brings every node's Position.  Callable wherever read_roots() is; reading changes nothing."""
        return tree_views(*self.read_tree_arrays(games, min_visits, max_depth, states))

    def read_pv(self, cap=64):
        """The principal variation of every game -> (list of move-index lists, q [G] f32, visits [G] u32):
        from the root the most visited move (ties to the larger index, self-play's rule), down while it has
        a child node, at most `cap` moves; q and visits are the first move's score / visits and visits."""
        moves = np.zeros((self.games, max(cap, 1)), np.int32)
        ln = np.zeros(self.games, np.int32)
        q = np.zeros(self.games, np.float32)
        vis = np.zeros(self.games, np.uint32)
        L.check(L.lib.az_search_read_pv(self._h, L.i32ptr(moves) if cap > 0 else None, int(cap), L.i32ptr(ln), L.fptr(q),
                                        L.u32ptr(vis)))
        return [moves[g, :ln[g]].tolist() for g in range(self.games)], q, vis

    def advance(self, actions, apply_noise=True):
        a = np.ascontiguousarray(actions, np.int32)
        res = np.zeros(self.games, np.int32)
        self.check(L.lib.az_search_advance(self._h, L.i32ptr(a), 1 if apply_noise else 0, L.i32ptr(res)))
        return res

    def adopt(self, apply_noise=False):
        """az_search_adopt_net: after the model was updated in place (or a caller-owned evaluator's
        model changed), rebuild every active root on the new weights -- the state set_roots would give
        from the game's history, game id and noise ply -- so that run() is valid again.  Inactive games
        keep their visits.  A no-op for a net whose generation has not moved."""
        self.check(L.lib.az_search_adopt_net(self._h, 1 if apply_noise else 0))

    @property
    def persistent(self):
        """True if the untimed simulation steps run through the persistent per-game kernel."""
        return bool(L.lib.az_search_persistent(self._h))

    @property
    def leaves(self):
        """Leaves per game per simulation step (make_cfg's `leaves`; 0 and 1 both read 1)."""
        k = C.c_int()
        L.check(L.lib.az_search_leaf_stats(self._h, C.byref(k), None))
        return k.value

    @property
    def shared_leaves(self):
        """Simulations whose leaf shared the expansion of an earlier leaf of its wave, since creation or
        the last SelfPlay.reset() (which clears every counter of stats() too).  stats()'s sims == evals +
        cache_hits + terminal_leaves + shared_leaves + the simulations selected onto an edge already known to
        end the game (terminal_leaves counts an ended game once, when an expansion finds it)."""
        n = C.c_uint64()
        L.check(L.lib.az_search_leaf_stats(self._h, None, C.byref(n)))
        return n.value

    def stats(self):
        s = L.AzSearchStats()
        L.check(L.lib.az_search_stats_get(self._h, C.byref(s)))
        return {k: getattr(s, k) for k, _ in s._fields_}

    def eval_log(self):
        nr, npri = C.c_int64(), C.c_int64()
        L.check(L.lib.az_search_eval_log(self._h, C.byref(nr), C.byref(npri), None, None, None, None, None))
        keys = np.zeros(max(nr.value, 1), np.uint64)
        vals = np.zeros(max(nr.value, 1), np.float32)
        off = np.zeros(nr.value + 1, np.int32)
        idx = np.zeros(max(npri.value, 1), np.int32)
        pri = np.zeros(max(npri.value, 1), np.float32)
        L.check(L.lib.az_search_eval_log(self._h, C.byref(nr), C.byref(npri), L.u64ptr(keys), L.fptr(vals),
                                         L.i32ptr(off), L.i32ptr(idx), L.fptr(pri)))
        n = nr.value
        return keys[:n], vals[:n], off, idx[:off[n]], pri[:off[n]]

    def timing(self, reset=False, enable=None):
        t = L.AzTiming()
        L.check(L.lib.az_search_timing(self._h, C.byref(t), 1 if reset else 0,
                                       1 if (enable if enable is not None else True) else 0))
        return {k: getattr(t, k) for k, _ in t._fields_}


class MCTree:
    """One game's search tree (tree.rs:25-269), backed by a 1-game BatchedSearch."""

    def __init__(self, search, history):
        self._s = search
        self.history = list(history)

    @classmethod
    def init(cls, model, state, apply_noise, **cfg):
        """MCTree::init (tree.rs:37-64): evaluate the root with `model`.  tree_reuse=True (in cfg):
        traverse_new keeps the played move's subtree (BatchedSearch)."""
        s = BatchedSearch(model, games=1, **cfg)
        hist = list(state.history())
        s.set_roots([hist], apply_noise=apply_noise)
        return cls(s, hist)

    def monte_carlo_tree_search(self):
        """tree.rs:106-115: run the simulations, return the improved policy [4096]."""
        imp, vis, dep = self._s.run()
        self.depth = int(dep[0])
        return imp[0]

    def view(self, states=True):
        """the tree as it stands on the device: its root TreeView (BatchedSearch.read_tree)"""
        return self._s.read_tree(games=[0], states=states)[0]

    # the reference's public fields (tree.rs:25-34), read from the device on access
    nodes = property(lambda self: self.view().nodes, doc="move index -> child TreeView")
    moves = property(lambda self: self.view(False).moves, doc="legal move indices, promotions four times")
    policy = property(lambda self: self.view(False).policy, doc="dense [4096] f32 priors")
    visits = property(lambda self: self.view(False).visits, doc="dense [4096] f32 visits")
    scores = property(lambda self: self.view(False).scores, doc="dense [4096] f32 scores")
    state = property(lambda self: self.view().state, doc="the root's Position")

    def max_subtree_depth(self):
        return self.depth

    def traverse_new(self, action, apply_noise):
        """tree.rs:239-256 (the action is also played on the tree's GameState)."""
        res = self._s.advance([action], apply_noise=apply_noise)
        self.history.append(int(action))
        return int(res[0])
