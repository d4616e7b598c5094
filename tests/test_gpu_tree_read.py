"""Whole-tree read-out (az_search_read_tree / az_search_read_pv) against the trees of
tests/treereuse_ref.py, compared by path with f32 fields as bit patterns: through both step forms, the
persistent kernel, mid-move, tree reuse's compaction, pruning, leaves > 1, the PV rule and the refusals.  The
cases' roots, the restatement's trees and the comparison live in tests/test_tree_read_host.py, which also
asserts the cases' own conditions (a draw, a win and a promotion edge within 32 simulations, a tie)."""
import ctypes as C

import numpy as np
import pytest

import azchess as A
import azchess._lib as L
import oracle as O
import treereuse_ref as R
from test_gpu_leafpar import log_evaluator
from test_tree_read_host import (DEEP_SIMS, ROOTS, SEED, SIMS, assert_same_tree, assert_well_formed, case_search,
                                 deep_search, flatten_view, host_position, noise_key, pv_ref, pv_view, start_of)

pytestmark = pytest.mark.gpu
F = np.float32
G = len(ROOTS)


def set_case_roots(s, noise, roots=ROOTS):
    s.set_roots([h for _, h in roots], apply_noise=noise,
                start=[A.Position.startpos() if f is None else A.Position.from_fen(f) for f, _ in roots])


def case_handle(noise, sims=SIMS, roots=ROOTS, **kw):
    s = A.BatchedSearch(None, games=len(roots), sims=sims, noise=noise, seed=SEED, cache_capacity=0, **kw)
    set_case_roots(s, noise, roots)
    return s


def assert_root_rows(s, views):
    """the export's root rows equal az_search_read_roots: visits, improved policy (bit patterns), depth"""
    imp, vis, dep = s.read_roots()
    for g, v in enumerate(views):
        assert np.array_equal(v.visits, vis[g].astype(F)), g
        tot = v.visits.sum(dtype=F)
        if tot > 0:
            assert np.array_equal((v.visits / tot).view(np.uint32), imp[g].view(np.uint32)), g
        assert v.max_subtree_depth() == dep[g] and v.nsum == int(vis[g].sum()), g


def last_max(vis_row):
    idx = np.nonzero(vis_row)[0]
    return int(max(zip(vis_row[idx].tolist(), idx.tolist()))[1])


# ------------------------------------------------------------------ 1. whole tree, every step form
@pytest.mark.parametrize("form", ["fused", "split", "persistent"])
@pytest.mark.parametrize("noise", [False, True])
def test_whole_tree_every_step_form(require_gpu, monkeypatch, noise, form):
    monkeypatch.setenv("AZ_FUSED_STEPS", "0" if form == "split" else "1")
    if form == "persistent":
        monkeypatch.setenv("AZ_PERSIST", "1")
        net = A.AlphaZero(6, 64, weights=A.random_weights(6, 64, seed=42), dtype="f32")
        s = A.BatchedSearch(net, games=G, sims=SIMS, noise=noise, seed=SEED, cache_capacity=0, record_evals=True,
                            eval_log_cap=1 << 13)
        assert s.persistent
        set_case_roots(s, noise)
    else:
        s = case_handle(noise)
        assert not s.persistent
    s.run()
    views = s.read_tree(states=True)
    assert len(views) == G
    if form == "persistent":
        ev = log_evaluator(s)
        refs = []
        for k, (fen, h) in enumerate(ROOTS):
            r = R.Search(h, ev, SIMS, noise_key(noise, k, len(h)), start=start_of(fen))
            r.run()
            refs.append(r.root)
    else:
        refs = [case_search(k, noise).root for k in range(G)]
    for k, (fen, h) in enumerate(ROOTS):
        assert_same_tree(views[k], refs[k], fen, h, (form, noise, k))
    assert_root_rows(s, views)
    assert s.stats()["overflow"] == 0


# ------------------------------------------------------------------ 2. one game at 512 simulations
def test_deep_tree_spans_several_chunks(require_gpu):
    s = case_handle(False, sims=DEEP_SIMS, roots=[(None, [])])
    s.run()
    views = s.read_tree(states=True)
    assert len(views[0]._nodes) > 4 * 64
    assert_same_tree(views[0], deep_search().root, None, [], "deep")
    assert_root_rows(s, views)


# ------------------------------------------------------------------ 3. mid-move
def test_mid_move_reads_change_nothing(require_gpu):
    cfg = dict(games=4, sims=16, seed=SEED, noise=True, cache_capacity=0)
    sp, twin = A.SelfPlay(None, **cfg), A.SelfPlay(None, **cfg)
    sp.reset()
    twin.reset()
    hist = [[] for _ in range(4)]
    for move in range(2):
        done, sims = False, 0
        while not done:
            done = sp.run_sims(5)[2]
            assert twin.run_sims(5)[2] == done
            sims = min(sims + 5, 16)
            views = sp.search.read_tree(states=True)
            if done:                                        # the move was played: the next root, nothing run on it
                hist = [h for _, _, _, _, h in sp.inflight()]
                assert all(len(h) == move + 1 for h in hist)
            for g in range(4):
                ref = R.Search(hist[g], O.synth_eval, sims, noise_key(True, g, len(hist[g])))
                if not done:
                    ref.run()
                assert_same_tree(views[g], ref.root, None, hist[g], (move, sims, g))
            assert_root_rows(sp.search, views)
    sp.run_sims(7)
    twin.run_sims(7)
    sp.search.read_tree()
    sp.search.read_pv()
    a, b = sp.search.read_roots(), twin.search.read_roots()
    assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b))
    assert sp.run_sims(16) == twin.run_sims(16) and sp.inflight() == twin.inflight()
    for _ in range(3):
        assert sp.step() == twin.step()
    assert sp.inflight() == twin.inflight() and sp.search.stats() == twin.search.stats()
    assert bytes(sp.drain_raw()) == bytes(twin.drain_raw())


# ------------------------------------------------------------------ 4. tree reuse on
@pytest.mark.parametrize("noise", [False, True])
def test_tree_reuse_export_is_the_kept_subtree(require_gpu, noise):
    roots = ROOTS[3:]
    s = case_handle(noise, roots=roots, tree_reuse=True)
    refs = [R.Search(h, O.synth_eval, SIMS, noise_key(noise, g, len(h))) for g, (_, h) in enumerate(roots)]
    hist = [list(h) for _, h in roots]
    for ply in range(3):
        _, vis, _ = s.run()
        for r in refs:
            r.run()
        views = s.read_tree(states=True)
        for g in range(len(roots)):
            assert_same_tree(views[g], refs[g].root, None, hist[g], ("run", ply, g))
        assert_root_rows(s, views)
        actions = [last_max(vis[g]) for g in range(len(roots))]
        assert actions == [r.last_max() for r in refs]
        assert s.advance(actions, apply_noise=noise).tolist() == [0] * len(roots)
        for g, r in enumerate(refs):
            hist[g].append(actions[g])
            assert r.advance(actions[g], noise_key(noise, g, len(hist[g]))) == 0
        views = s.read_tree(states=True)                    # the compaction's output, node for node
        for g in range(len(roots)):
            assert_same_tree(views[g], refs[g].root, None, hist[g], ("advance", ply, g))
    assert s.reuse_stats()["carried_nodes"] > 3 * len(roots)


# ------------------------------------------------------------------ 5. pruning
def prune_on_host(noff, eoff, nodes, edges, states, min_visits, max_depth):
    """the definition on the full export: a child node stays iff its parent does, its edge has visits >=
    min_visits and its depth is <= max_depth; a dropped child's edge reads AZ_TREE_CUT"""
    on, oe, os_, no, eo = [], [], [], [0], [0]
    for k in range(len(noff) - 1):
        n, e = nodes[noff[k]:noff[k + 1]], edges[eoff[k]:eoff[k + 1]]
        st = states[noff[k]:noff[k + 1]]
        new = np.full(len(n), -1)
        kept = []
        for i in range(len(n)):
            if i:
                p = n["parent"][i]
                pe = e[n["edge_begin"][p] + n["parent_edge"][i]]
                if new[p] < 0 or pe["visits"] < min_visits or (max_depth >= 0 and n["depth"][i] > max_depth):
                    continue
            new[i] = len(kept)
            kept.append(i)
        nn, ee = n[kept].copy(), []
        at = 0
        for j, i in enumerate(kept):
            rows = e[n["edge_begin"][i]:n["edge_begin"][i] + n["nedges"][i]].copy()
            ch = rows["child"]
            rows["child"] = np.where(ch >= 0, np.where(new[np.maximum(ch, 0)] >= 0, new[np.maximum(ch, 0)], L.TREE_CUT), ch)
            nn["edge_begin"][j] = at
            nn["parent"][j] = new[n["parent"][i]] if i else -1
            at += len(rows)
            ee.append(rows)
        on.append(nn)
        oe.append(np.concatenate(ee))
        os_.append(st[kept])
        no.append(no[-1] + len(nn))
        eo.append(eo[-1] + at)
    return np.array(no), np.array(eo), np.concatenate(on), np.concatenate(oe), np.concatenate(os_)


@pytest.mark.parametrize("min_visits,max_depth", [(2, None), (0, 1), (0, 0), (2, 1)])
def test_pruning_is_the_full_export_filtered(require_gpu, min_visits, max_depth):
    s = case_handle(True)
    s.run()
    full = s.read_tree_arrays(states=True)
    got = s.read_tree_arrays(min_visits=min_visits, max_depth=max_depth, states=True)
    want = prune_on_host(*full, min_visits, -1 if max_depth is None else max_depth)
    for name, a, b in zip(("node_off", "edge_off", "nodes", "edges", "states"), got, want):
        assert len(a) == len(b) and a.tobytes() == b.astype(a.dtype).tobytes(), name
    assert len(got[2]) < len(full[2]) and (got[3]["child"] == L.TREE_CUT).sum() > 0
    assert (full[3]["child"] == L.TREE_CUT).sum() == 0
    if max_depth == 0:
        assert len(got[2]) == G and (got[3]["child"] >= 0).sum() == 0
    for v in A.tree_views(*got):
        assert_well_formed(v)
        assert all(v.visits[i] > 0 for i in v.cut)
    # the sizing call's offsets are the real call's
    noff, eoff = np.full(G + 1, -1, np.int64), np.full(G + 1, -1, np.int64)
    p64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))
    L.check(L.lib.az_search_read_tree(s._h, None, G, min_visits, -1 if max_depth is None else max_depth, p64(noff),
                                      p64(eoff), None, 0, None, 0, None))
    assert np.array_equal(noff, got[0]) and np.array_equal(eoff, got[1])


# ------------------------------------------------------------------ 6. leaves = 4
@pytest.mark.parametrize("fused", ["1", "0"])
def test_leaf_parallel_tree_invariants(require_gpu, monkeypatch, fused):
    monkeypatch.setenv("AZ_FUSED_STEPS", fused)
    s = case_handle(True, leaves=4)
    assert s.leaves == 4
    s.run()
    views = s.read_tree(states=True)
    assert_root_rows(s, views)
    for k, (fen, h) in enumerate(ROOTS):
        assert_well_formed(views[k], k)
        flat = flatten_view(views[k])
        assert len(flat) == len(views[k]._nodes) > 1
        for path, rec in sorted(flat.items(), key=lambda t: len(t[0])):
            assert rec["nsum"] == sum(rec["visits"]) and rec["depth"] == len(path), (k, path)
            if path:
                par = flat[path[:-1]]
                e = par["index"].index(path[-1])
                assert par["visits"][e] >= 1 + rec["nsum"], (k, path)
            # the state: the parent's with the edge's move played, by the engine's host rules and the oracle's
            assert rec["state"] == host_position(fen, list(h) + list(path)).raw(), (k, path)
            g = O.Game(start_of(fen))
            for a in list(h) + list(path):
                assert g.play_index(int(a)) == 0
            assert rec["fen"] == O.to_fen(g.position), (k, path)
        assert flat[()]["nsum"] == SIMS


def test_one_leaf_visits_are_one_plus_the_childs(require_gpu):
    """K = 1: the visit that made a child node is the only one of its edge that is not in the child's nsum"""
    s = case_handle(False)
    s.run()
    for v in s.read_tree():
        flat = flatten_view(v, with_state=False)
        for path, rec in flat.items():
            if path:
                par = flat[path[:-1]]
                assert par["visits"][par["index"].index(path[-1])] == 1 + rec["nsum"]


# ------------------------------------------------------------------ 7. PV
@pytest.mark.parametrize("noise", [False, True])
def test_pv_follows_the_stated_rule(require_gpu, noise):
    s = case_handle(noise)
    s.run()
    views = s.read_tree()
    for cap in (64, 1, 0):
        moves, q, vis = s.read_pv(cap)
        for k in range(G):
            ref = pv_ref(case_search(k, noise).root, cap)
            exp = pv_view(views[k], cap)
            assert moves[k] == ref[0] == exp[0], (cap, k)
            assert F(q[k]).view(np.uint32) == F(ref[1]).view(np.uint32) == F(exp[1]).view(np.uint32), (cap, k)
            assert int(vis[k]) == ref[2] == exp[2], (cap, k)
        if cap == 64:
            assert max(len(m) for m in moves) > 1


def test_pv_takes_the_larger_index_on_a_tie(require_gpu):
    """a root whose two most visited edges tie (the host file asserts the cases hold one)"""
    found = 0
    for noise in (False, True):
        s = case_handle(noise)
        s.run()
        moves, _, vis = s.read_pv(1)
        for k, v in enumerate(s.read_tree(max_depth=0)):
            e = v.edges
            best = e["visits"].max()
            tied = e["index"][e["visits"] == best]
            if len(tied) > 1:
                found += 1
                assert moves[k] == [int(tied.max())] and vis[k] == best, (noise, k)
    assert found >= 1


# ------------------------------------------------------------------ 8. refusals and edges
def raw_read(s, games, n, min_visits, max_depth, node_cap, edge_cap, with_nodes=True, with_edges=True):
    """one raw call on pattern-filled outputs -> (rc, outputs)"""
    noff, eoff = np.full(16, -7, np.int64), np.full(16, -7, np.int64)
    nodes = np.zeros(max(node_cap, 1), L.TREE_NODE_DTYPE)
    edges = np.zeros(max(edge_cap, 1), L.TREE_EDGE_DTYPE)
    states = np.zeros(max(node_cap, 1), L.POS_DTYPE)
    for a in (nodes, edges, states):
        a.view(np.uint8)[:] = 0xA5
    gl = None if games is None else np.ascontiguousarray(games, np.int32)
    rc = L.lib.az_search_read_tree(
        s._h, None if gl is None else L.i32ptr(gl), n, min_visits, max_depth,
        noff.ctypes.data_as(C.POINTER(C.c_int64)), eoff.ctypes.data_as(C.POINTER(C.c_int64)),
        nodes.ctypes.data_as(C.POINTER(L.AzTreeNode)) if with_nodes else None, node_cap,
        edges.ctypes.data_as(C.POINTER(L.AzTreeEdge)) if with_edges else None, edge_cap,
        states.ctypes.data_as(C.POINTER(L.AzPos)))
    return rc, (noff, eoff, nodes, edges, states)


def untouched(outs):
    noff, eoff, nodes, edges, states = outs
    return ((noff == -7).all() and (eoff == -7).all()
            and all((a.view(np.uint8) == 0xA5).all() for a in (nodes, edges, states)))


def test_refusals_leave_the_outputs_untouched(require_gpu):
    s = case_handle(False)
    s.run()
    noff, eoff, nodes, edges, _ = s.read_tree_arrays(games=[0, 3])
    nn, ne = len(nodes), len(edges)
    for what, args in (("slot == G", ([0, G], 2, 0, -1, nn + 999, ne + 999)),
                       ("slot < 0", ([-1, 0], 2, 0, -1, nn + 999, ne + 999)),
                       ("n < 0", ([0, 3], -1, 0, -1, nn, ne)),
                       ("min_visits < 0", ([0, 3], 2, -1, -1, nn, ne)),
                       ("node_cap", ([0, 3], 2, 0, -1, nn - 1, ne)),
                       ("edge_cap", ([0, 3], 2, 0, -1, nn, ne - 1))):
        rc, outs = raw_read(s, *args)
        assert rc < 0 and L.lib.az_last_error(), what
        assert untouched(outs), what
    for what, kw in (("nodes NULL", dict(with_nodes=False)), ("edges NULL", dict(with_edges=False))):
        rc, outs = raw_read(s, [0, 3], 2, 0, -1, nn, ne, **kw)
        assert rc < 0 and untouched(outs), what
    # exact capacities are enough
    rc, outs = raw_read(s, [0, 3], 2, 0, -1, nn, ne)
    assert rc == 0 and outs[0][:3].tolist() == noff.tolist() and outs[1][:3].tolist() == eoff.tolist()
    assert outs[2][:nn].tobytes() == nodes.tobytes() and outs[3][:ne].tobytes() == edges.tobytes()
    assert (outs[0][3:] == -7).all()
    # n = 0 succeeds and writes the one offset
    rc, outs = raw_read(s, [0], 0, 0, -1, 4, 4)
    assert rc == 0 and outs[0][0] == 0 and outs[1][0] == 0 and (outs[0][1:] == -7).all()
    assert (outs[2].view(np.uint8) == 0xA5).all()
    # reading changed nothing
    views = s.read_tree(states=True)
    for k, (fen, h) in enumerate(ROOTS):
        assert_same_tree(views[k], case_search(k, False).root, fen, h, k)


def test_a_repeated_slot_exports_twice(require_gpu):
    s = case_handle(True)
    s.run()
    noff, eoff, nodes, edges, states = s.read_tree_arrays(games=[2, 5, 2], states=True)
    one = s.read_tree_arrays(games=[2], states=True)
    for a, off in ((nodes, noff), (edges, eoff), (states, noff)):
        assert a[off[0]:off[1]].tobytes() == a[off[2]:off[3]].tobytes()
    assert nodes[noff[0]:noff[1]].tobytes() == one[2].tobytes() and edges[eoff[0]:eoff[1]].tobytes() == one[3].tobytes()
    views = A.tree_views(noff, eoff, nodes, edges, states)
    for v, k in zip(views, (2, 5, 2)):
        assert_same_tree(v, case_search(k, True).root, *ROOTS[k], k)


def test_inactive_game_and_mctree_fields(require_gpu):
    # game 0 plays its mate and goes inactive: its arena still holds the tree it had, its root row is read_roots'
    s = case_handle(False)
    _, vis, _ = s.run()
    actions = [last_max(vis[g]) for g in range(G)]
    res = s.advance(actions, apply_noise=False)
    assert res[0] in (2, 3) and res[3] == 0
    views = s.read_tree(states=True)
    assert_root_rows(s, views)
    assert_same_tree(views[0], case_search(0, False).root, *ROOTS[0], "inactive")
    moves, q, v = s.read_pv(4)
    assert moves[0] == [actions[0]] and moves[3] == [] and q[3] == 0 and v[3] == 0
    # MCTree: the reference's fields, read from its one game
    state = A.GameState()
    t = A.MCTree.init(None, state, False, sims=SIMS, seed=SEED, cache_capacity=0)
    t.monte_carlo_tree_search()
    view = t._s.read_tree(states=True)[0]
    ref = case_search(3, False).root
    assert_same_tree(view, ref, None, [], "mctree")
    assert t.moves.tolist() == view.moves.tolist() == [int(i) for i in ref.all_idx]
    for name in ("policy", "visits", "scores"):
        assert np.array_equal(getattr(t, name).view(np.uint32), getattr(view, name).view(np.uint32)), name
    assert t.state == A.Position.startpos() and set(t.nodes) == set(view.nodes)
    child = t.nodes[last_max(t.visits)]
    assert child.depth == 1 and child.state == A.Position.startpos().play(last_max(t.visits))
