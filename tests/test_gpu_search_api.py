"""The stepwise search API (az_search_advance, az_search_read_roots mid-move), every search setting
away from the reference's defaults, the size at which the persistent kernel switches itself on and
az_net_forward_device on a caller's stream -- against the oracle, BIT-EXACT (visits, improved
policies, depths, result codes).  The conditions on the inputs (the advance identity, the scenario
table) are asserted from the oracle alone in tests/test_oracle_search_api.py."""
import numpy as np
import pytest

import azchess as A
import oracle as O
import test_oracle_search_api as T
from azchess import _lib as L
from test_gpu_rules import _valid_histories
from test_gpu_search import compare_steps, histories

pytestmark = pytest.mark.gpu

ONGOING, ILLEGAL = T.ONGOING, T.ILLEGAL


def assert_root(got, g, ref, what):
    """game g of (improved, visits, depth) against the oracle's (visits, improved, depth, ...)"""
    imp, vis, dep = got
    assert np.array_equal(vis[g].astype(np.float32), ref[0]), what
    assert np.array_equal(imp[g], ref[1]), what
    assert dep[g] == ref[2], what


def assert_unvisited(got, g, legal, what):
    """game g stands on a root no simulation has visited: visits and depth 0, improved 0 / 0 = NaN at
    exactly the root's legal move indices and 0 elsewhere (include/az.h, az_search_read_roots)"""
    imp, vis, dep = got
    assert not vis[g].any() and dep[g] == 0, what
    mask = np.zeros(4096, bool)
    mask[np.asarray(sorted(set(legal)), np.int64)] = True
    assert np.array_equal(np.isnan(imp[g]), mask) and not imp[g][~mask].any(), what


def kth_most_visited(vis, k):
    """the k-th most visited move (ties: the smaller index first), the last one if there are fewer"""
    order = sorted(np.nonzero(vis)[0].tolist(), key=lambda a: (-vis[a], a))
    return int(order[min(k, len(order) - 1)])


# ------------------------------------------------------------------ 1. az_search_advance
@pytest.mark.parametrize("noise", [False, True])
@pytest.mark.parametrize("fused", ["1", "0"])
def test_advance_matches_fresh_search(require_gpu, monkeypatch, fused, noise):
    """k_finish in mode 1 (traverse_new with the caller's actions, tree.rs:239-256) on one game per
    scenario row: a move that ends the game (mate for either side, 50-move, fullmove 200, threefold,
    stalemate), a legal move that was never expanded, indices that are no move, and ongoing moves
    (most / least visited child, promotion, castling, en passant).  Result codes equal the table; a
    game whose result is not AZ_ONGOING is inactive (no simulation runs or is counted for it, its
    outputs stay frozen, a further advance answers AZ_ILLEGAL); every ongoing game's next run equals
    the oracle's fresh search of the extended history with the noise stream of ply + 1, over four
    plies in all (the k-th most visited child, k cycling 0, 1, 2)."""
    monkeypatch.setenv("AZ_FUSED_STEPS", fused)
    rows = T.scenario_rows(noise)
    G, S, seed = len(rows), T.SIMS, T.SEED
    cfg = O.make_cfg(sims=S, noise=noise, seed=seed, eval_kind=0)
    s = A.BatchedSearch(None, games=G, sims=S, noise=noise, seed=seed, cache_capacity=0)
    s.set_roots([r.history for r in rows], apply_noise=noise, start=[A.Position.from_fen(r.fen) for r in rows])
    got = s.read_roots()                                             # fresh roots: nothing visited yet
    for g, r in enumerate(rows):
        assert_unvisited(got, g, r.legal, r.name)
    sims0 = s.stats()["sims"]
    first = s.run()
    for g, r in enumerate(rows):
        assert_root(first, g, (r.visits, r.improved, r.depth), r.name)
    assert s.stats()["sims"] - sims0 == G * S
    res = s.advance([r.action for r in rows], apply_noise=noise)
    assert res.tolist() == [r.expected for r in rows]
    hist = {g: list(r.history) + [r.action] for g, r in enumerate(rows) if r.expected == ONGOING}
    assert sorted(rows[g].name for g in hist) == ["i", "j", "k", "l", "m"]
    # zero-simulation read right after the advance: the re-rooted games are unvisited, the others stay
    got = s.read_roots()
    for g in range(G):
        if g in hist:
            assert_unvisited(got, g, O.legal_indices(T.game_at(rows[g].fen, hist[g]).position).tolist(), rows[g].name)
        else:
            assert_root(got, g, (rows[g].visits, rows[g].improved, rows[g].depth), rows[g].name)
    for ply in range(4):
        sims0 = s.stats()["sims"]
        got = s.run()
        assert s.stats()["sims"] - sims0 == len(hist) * S            # active games only
        refs = {}
        for g in range(G):
            r = rows[g]
            if g in hist:
                key = O.lib().ref_stream_key(seed, g, len(hist[g]), 0)
                refs[g] = O.search_game(cfg, hist[g], noise=noise, noise_key=key, start=O.from_fen(r.fen))
                assert_root(got, g, refs[g], (r.name, ply))
            else:                                                     # frozen at its last root
                assert_root(got, g, (r.visits, r.improved, r.depth), (r.name, ply))
        assert [np.array_equal(a, b) for a, b in zip(s.read_roots(), got)] == [True] * 3
        if ply == 3:
            break
        actions, want = [0] * G, [ILLEGAL] * G                       # an inactive game: AZ_ILLEGAL again
        for g in hist:
            actions[g] = kth_most_visited(refs[g][0], ply % 3)
            want[g] = T.play_result(rows[g].fen, hist[g], actions[g])
        res = s.advance(actions, apply_noise=noise)
        assert res.tolist() == want, ply
        hist = {g: h + [actions[g]] for g, h in hist.items() if want[g] == ONGOING}
        assert len(hist) >= 3
    # new roots make every game active again
    s.set_roots([r.history for r in rows], apply_noise=noise, start=[A.Position.from_fen(r.fen) for r in rows])
    sims0 = s.stats()["sims"]
    again = s.run()
    assert s.stats()["sims"] - sims0 == G * S
    assert [np.array_equal(a, b) for a, b in zip(again, first)] == [True] * 3
    assert s.stats()["overflow"] == 0


# ------------------------------------------------------------------ 2. the FEN cache across a re-root
def test_advance_with_the_fen_cache(require_gpu):
    """The ongoing rows at 200 simulations with the FEN cache on and off: identical results, equal to
    the oracle, and the searches after a re-root are served entries inserted before it (the re-root
    drops the grandchildren, so the next search expands positions the cache already holds)."""
    S, seed = 200, T.SEED
    ids = [g for g, r in enumerate(T.scenario_rows(True)) if r.expected == ONGOING]
    rows = [T.scenario_rows(True)[g] for g in ids]       # visited at 64 simulations, so at 200 (a prefix)
    cfg = O.make_cfg(sims=S, noise=True, seed=seed, eval_kind=0)
    hists = [list(r.history) for r in rows]
    actions = [r.action for r in rows]
    runs = {0: [], 1 << 16: []}
    hits = []
    for move in range(3):
        refs = [O.search_game(cfg, h, noise=True, noise_key=O.lib().ref_stream_key(seed, g, len(h), 0),
                              start=O.from_fen(r.fen)) for g, h, r in zip(ids, hists, rows)]
        if move > 0:
            actions = [kth_most_visited(ref[0], 0) for ref in refs]
        for cap, out in runs.items():
            if move == 0:
                s = A.BatchedSearch(None, games=len(rows), sims=S, noise=True, seed=seed, cache_capacity=cap)
                s.set_roots(hists, apply_noise=True, game_ids=ids, start=[A.Position.from_fen(r.fen) for r in rows])
                out.append(s)
            s = out[0]
            got = s.run()
            for k, ref in enumerate(refs):
                assert_root(got, k, ref, (cap, move, rows[k].name))
            want = [T.play_result(r.fen, h, a) for r, h, a in zip(rows, hists, actions)]
            assert want == [ONGOING] * len(rows)
            assert s.advance(actions, apply_noise=True).tolist() == want
            if cap:
                hits.append(s.stats()["cache_hits"])
        hists = [h + [a] for h, a in zip(hists, actions)]
    assert runs[0][0].stats()["cache_hits"] == 0
    assert hits[1] > hits[0] and hits[2] > hits[1]       # the searches after a re-root hit the cache
    assert runs[1 << 16][0].stats()["overflow"] == 0


# ------------------------------------------------------------------ 3. advance with a network
@pytest.mark.parametrize("blocks,filters,dtype,persist", [(6, 64, "f32", True), (2, 32, "bf16", False)])
def test_advance_with_a_network(require_gpu, monkeypatch, blocks, filters, dtype, persist):
    """run, advance by a visited child that is not the most visited one, run -- against a fresh handle
    rooted at the extended histories (same seed and game ids, so the same noise): bit-identical
    visits, improved policies and depths (a child's search-mode evaluation equals its root
    evaluation), both reproduced by the oracle replaying the handle's evaluations.  6x64 f32 through
    the persistent kernel (run after a re-root, with an inactive game in the batch), 2x32 bf16 through
    the step kernels."""
    if persist:
        monkeypatch.setenv("AZ_PERSIST", "1")
    S, seed, shift = 64, 19, 3
    hs = histories(8, 5)
    net = A.AlphaZero(blocks, filters, weights=A.random_weights(blocks, filters, seed=42), dtype=dtype)
    mk = lambda games: A.BatchedSearch(net, games=games, sims=S, seed=seed, cache_capacity=0, record_evals=True,
                                       eval_log_cap=1 << 15)
    # handle A: the 8 games and a ninth that an action that is no move takes out; noise plies `shift`
    # past the history lengths (az_search_set_roots' noise_ply; each advance adds one)
    a = mk(len(hs) + 1)
    assert a.persistent == persist
    a.set_roots(hs + [[]], apply_noise=True, noise_plies=[len(h) + shift for h in hs + [[]]])
    first = a.run()
    vis = first[1]
    actions = []
    for g, h in enumerate(hs):
        c = [x for x in sorted(np.nonzero(vis[g])[0].tolist(), key=lambda x: (vis[g][x], x))
             if vis[g][x] < vis[g].max() and T.play_result(T.START_FEN, h, x) == ONGOING]
        actions.append(int(c[0]))                      # the least visited ongoing child
    sims0 = a.stats()["sims"]
    assert a.advance(actions + [-1], apply_noise=True).tolist() == [ONGOING] * len(hs) + [ILLEGAL]
    got_a = a.run()
    assert a.stats()["sims"] - sims0 == len(hs) * S    # the inactive game runs nothing in either kernel
    for x, y in zip(got_a, first):
        assert np.array_equal(x[len(hs)], y[len(hs)])  # and stays frozen
    ext = [h + [x] for h, x in zip(hs, actions)]
    b = mk(len(hs))
    b.set_roots(ext, apply_noise=True, noise_plies=[len(h) + shift for h in ext])
    got_b = b.run()
    for x, y in zip(got_a, got_b):
        assert np.array_equal(x[:len(hs)], y)
    cfg = O.make_cfg(sims=S, noise=True, seed=seed, eval_kind=2)
    for s, got in ((a, got_a), (b, got_b)):
        rep = O.Replay(*s.eval_log())
        for g, h in enumerate(ext):
            key = O.lib().ref_stream_key(seed, g, len(h) + shift, 0)
            rv, ri, rd, _ = O.search_game(cfg, h, noise=True, noise_key=key, replay=rep)
            assert_root(got, g, (rv, ri, rd), g)
        assert s.stats()["overflow"] == 0


# ------------------------------------------------------------------ 4. the MCTree mirror
def test_mctree_mirror_plays_a_short_game(require_gpu):
    """azchess.MCTree (init -> monte_carlo_tree_search -> traverse_new, the reference's method names)
    for 6 plies: every ply's improved policy and max_subtree_depth equal the oracle's search of the
    history so far."""
    S, seed = 32, 7
    cfg = O.make_cfg(sims=S, noise=True, seed=seed, eval_kind=0)
    state = A.GameState()
    assert int(A.play_move(state, 588)) == ONGOING
    t = A.MCTree.init(None, state, True, sims=S, seed=seed, cache_capacity=0)
    for ply in range(6):
        h = list(t.history)
        assert len(h) == 1 + ply
        imp = t.monte_carlo_tree_search()
        rv, ri, rd, _ = O.search_game(cfg, h, noise=True, noise_key=O.lib().ref_stream_key(seed, 0, len(h), 0))
        assert np.array_equal(imp, ri), ply
        assert np.array_equal(t.visits, rv) and t.max_subtree_depth() == rd, ply
        action = kth_most_visited(rv, ply % 3)
        assert T.play_result(T.START_FEN, h, action) == ONGOING
        assert t.traverse_new(action, True) == ONGOING


# ------------------------------------------------------------------ 5. az_search_read_roots mid-move
CHUNKS = (1, 7, 24, 1, 31, 36)          # cumulative 1, 8, 32, 33, 64, 100: on and off the timed steps


def _read_roots_mid_move(net, timing, play_out):
    G, S, seed = 8, 100, 37
    mk = lambda: A.SelfPlay(net, games=G, sims=S, seed=seed, cache_capacity=0, record_evals=net is not None,
                            eval_log_cap=1 << 16 if net is not None else 0)
    sp, twin = mk(), mk()
    for x in (sp, twin):
        x.reset()
        x.search.timing(reset=True, enable=timing)
    # zero-simulation read before the first chunk
    got = sp.search.read_roots()
    for g in range(G):
        assert_unvisited(got, g, O.legal_indices(O.startpos()).tolist(), g)
    cum = 0
    for k in CHUNKS:
        fin, active, done = sp.run_sims(k)
        cum += k
        assert done == (cum == S)
        if done:
            break
        got = sp.search.read_roots()
        assert np.all(got[1].sum(1) == cum), cum
        cfg = O.make_cfg(sims=cum, noise=True, seed=seed, eval_kind=0 if net is None else 2)
        rep = O.Replay(*sp.search.eval_log()) if net is not None else None
        for g in range(G):
            ref = O.search_game(cfg, [], noise=True, noise_key=O.lib().ref_stream_key(seed, g, 0, 0), replay=rep)
            assert_root(got, g, ref, (cum, g))
    assert cum == S and active == G
    # right after the completed move every game stands on a root no simulation has visited: one ply
    # from the start position, where Black has 20 legal moves whatever White played
    imp, vis, dep = sp.search.read_roots()
    assert not vis.any() and not dep.any()
    assert np.all(np.isnan(imp).sum(1) == 20) and not imp[~np.isnan(imp)].any()
    # reading did not disturb the move: the twin played it in one undisturbed step
    assert twin.step() == (fin, active)
    steps = []
    for x in (sp, twin):
        if play_out:                                 # to the end of every game: all EpisodeSteps
            for _ in range(1000):
                if x.step()[1] == 0:
                    break
        else:                                        # into the next move: the same root, the same search
            assert x.run_sims(S - 1)[2] is False
        st = x.search.stats()
        steps.append(((st["sims"], st["evals"], st["terminal_leaves"], st["moves"], st["overflow"]),
                      sorted((s.game_id, s.ply, s.action, s.search_depth, s.result, np.float32(s.final_value),
                              tuple(sorted(s.visits.items()))) for s in x.drain()),
                      [a.tobytes() for a in x.search.read_roots()]))
    assert steps[0] == steps[1]
    assert steps[0][0][4] == 0 and (len(steps[0][1]) > G) == play_out
    if play_out and net is None:                     # the chunked move itself, complete: the oracle's 100 simulations
        cfg = O.make_cfg(sims=S, noise=True, seed=seed, eval_kind=0)
        first = {s[0]: s for s in steps[0][1] if s[1] == 0}
        for g in range(G):
            rv, _, rd, _ = O.search_game(cfg, [], noise=True, noise_key=O.lib().ref_stream_key(seed, g, 0, 0))
            assert dict(first[g][6]) == {int(i): int(rv[i]) for i in np.nonzero(rv)[0]} and first[g][3] == rd, g


@pytest.mark.parametrize("fused", ["1", "0"])
def test_read_roots_mid_move_synthetic(require_gpu, monkeypatch, fused):
    """az_search_read_roots after every chunk of a move cut by az_selfplay_run_sims (with k_step the
    backup of simulation i rides in the launch of i + 1 and is flushed at the chunk's end): the roots
    are exactly the oracle's tree after the cumulative number of simulations -- no backup pending,
    none counted twice -- and reading does not disturb the move: the games played to their end give
    the EpisodeSteps of a twin handle that played the move in one step().  Zero-simulation reads
    (before the first chunk, right after the completed move): visits and depth 0, improved NaN at the
    root's legal moves."""
    monkeypatch.setenv("AZ_FUSED_STEPS", fused)
    _read_roots_mid_move(None, False, play_out=True)


@pytest.mark.parametrize("timing", [False, True])
@pytest.mark.parametrize("fused", ["1", "0"])
@pytest.mark.parametrize("persist", ["1", "0"])
def test_read_roots_mid_move_net(require_gpu, monkeypatch, persist, fused, timing):
    """The same with the 6x64 f32 net, through the persistent kernel (a chunk is one launch) and the
    step kernels, fused or not, with and without the every-32nd timed step: the oracle replays the
    handle's evaluations up to each chunk edge.  The twin comparison runs into the next move (the
    same root and the same 99 simulations there) instead of to the games' ends: played out with the
    net a case takes 7 s, and the synthetic cases above do play to the ends through the step kernels."""
    monkeypatch.setenv("AZ_PERSIST", persist)
    monkeypatch.setenv("AZ_FUSED_STEPS", fused)
    net = A.AlphaZero(6, 64, weights=A.random_weights(6, 64, seed=42), dtype="f32")
    _read_roots_mid_move(net, timing, play_out=False)


# ------------------------------------------------------------------ 6. search settings
DEFAULTS = dict(dir_alpha=0.3, dir_eps=0.25, c_puct=3.0, temp_moves=15)
SEARCH_SETTINGS = (
    [dict(DEFAULTS, dir_alpha=a, dir_eps=e) for a, e in ((1.0, 0.25), (2.5, 1.0), (0.03, 0.25), (0.3, 0.0))]
    + [dict(DEFAULTS, c_puct=c) for c in (0.5, 10.0)]
    + [dict(DEFAULTS, temp_moves=t) for t in (0, 3, 1000)]
    + [dict(dir_alpha=2.5, dir_eps=1.0, c_puct=0.5, temp_moves=1000),
       dict(dir_alpha=0.03, dir_eps=0.0, c_puct=10.0, temp_moves=3)])


@pytest.mark.parametrize("setting", SEARCH_SETTINGS, ids=lambda d: "a%(dir_alpha)g-e%(dir_eps)g-c%(c_puct)g-t%(temp_moves)d" % d)
def test_search_settings_match_oracle(require_gpu, setting):
    """Every search setting away from the reference's defaults, one factor at a time and two mixed:
    Dirichlet alpha below and above 1 (gamma_sample's shape >= 1 branch), epsilon 0 and 1, a small and
    a large c_puct, temp_moves 0 (always the last maximum), 3 and 1000 (always WeightedIndex).  Whole
    self-play games equal the oracle's step for step, and one search of the edge-position roots equals
    the oracle's."""
    ocfg = dict(c_puct=setting["c_puct"], alpha=setting["dir_alpha"], eps=setting["dir_eps"],
                temp_moves=setting["temp_moves"])
    ref, _, _ = O.selfplay(O.make_cfg(sims=16, noise=True, seed=5, eval_kind=0, **ocfg), 3)
    # the setting bites (from the oracle's steps alone)
    last_max = [max(a for a, n in s["visits"].items() if n == max(s["visits"].values())) for s in ref]
    if setting["temp_moves"] == 0:
        assert [s["action"] for s in ref] == last_max
    if setting["temp_moves"] == 1000:
        assert any(s["visits"][s["action"]] < max(s["visits"].values()) for s in ref)
    _, steps = A.run_all_episodes(None, games=3, sims=16, seed=5, **setting)
    compare_steps(steps, ref)
    roots = _valid_histories()
    S, seed = 64, 23
    s = A.BatchedSearch(None, games=len(roots), sims=S, noise=True, seed=seed, cache_capacity=0, **setting)
    s.set_roots([h for _, h in roots], apply_noise=True, start=[A.Position.from_fen(f) for f, _ in roots])
    got = s.run()
    cfg = O.make_cfg(sims=S, noise=True, seed=seed, eval_kind=0, **ocfg)
    quiet = O.make_cfg(sims=S, noise=False, seed=seed, eval_kind=0, **ocfg)
    for g, (fen, h) in enumerate(roots):
        ref = O.search_game(cfg, h, noise=True, noise_key=O.lib().ref_stream_key(seed, g, len(h), 0),
                            start=O.from_fen(fen))
        assert_root(got, g, ref, fen)
        if setting["dir_eps"] == 0.0:                # the noise is weighted away: the noise-off search
            off = O.search_game(quiet, h, noise=False, start=O.from_fen(fen))
            assert np.array_equal(ref[0], off[0]) and np.array_equal(ref[1], off[1]) and ref[2] == off[2]
    assert s.stats()["overflow"] == 0


# ------------------------------------------------------------------ 7. the persistent kernel's switch
def test_persistent_switches_at_the_cu_count(require_gpu, monkeypatch):
    """AZ_PERSIST unset: the persistent per-game kernel runs when the games fit the device in one
    round (G <= compute units) and the step kernels one game above; games 0..C-1 of the two runs are
    bit-identical, and the oracle replay reproduces 4 sampled games of each."""
    from azchess.hiprt import Hip
    monkeypatch.delenv("AZ_PERSIST", raising=False)
    # the device's compute units from the HIP runtime libaz is bound to (torch.cuda finds no device in a
    # process where libaz has loaded /opt/rocm's runtime first)
    C = Hip().multiprocessor_count(0)
    assert C >= 4
    S, seed = 24, 3
    net = A.AlphaZero(6, 64, weights=A.random_weights(6, 64, seed=42), dtype="f32")
    cfg = O.make_cfg(sims=S, noise=True, seed=seed, eval_kind=2)
    runs = []
    for G, want in ((C, True), (C + 1, False)):
        s = A.BatchedSearch(net, games=G, sims=S, seed=seed, cache_capacity=0, record_evals=True,
                            eval_log_cap=(G + 1) * (S + 1))
        assert s.persistent == want, G
        s.set_roots([[]] * G, apply_noise=True)
        got = s.run()
        assert np.all(got[1].sum(1) == S) and s.stats()["overflow"] == 0
        rep = O.Replay(*s.eval_log())
        for g in (0, 1, C // 2, C - 1):
            ref = O.search_game(cfg, [], noise=True, noise_key=O.lib().ref_stream_key(seed, g, 0, 0), replay=rep)
            assert_root(got, g, ref, (G, g))
        runs.append(got)
    for x, y in zip(*runs):
        assert np.array_equal(x[:C], y[:C])


# ------------------------------------------------------------------ 8. az_net_forward_device
@pytest.mark.parametrize("blocks,filters,dtype", [(2, 32, "f32"), (6, 64, "bf16"), (2, 256, "f32")])
def test_forward_device_equals_forward(require_gpu, blocks, filters, dtype):
    """az_net_forward_device on the caller's device buffers, on the engine stream (NULL) and on a
    caller's stream, at n = 33, 1, 5 on the same buffers (NaN-filled between calls): rows [0, n) equal
    az_net_forward bit for bit, policy rows sum to 1, and nothing past row n is written -- a call with
    a smaller n after a larger one leaves no stale row behind."""
    from azchess.hiprt import Hip
    hip = Hip()
    NMAX = 33
    net = A.AlphaZero(blocks, filters, weights=A.random_weights(blocks, filters, seed=42), dtype=dtype)
    rng = np.random.default_rng(8)
    planes = []
    for h in histories(NMAX, 3):
        p = A.Position.startpos()
        for a in h:
            p = p.play(a)
        planes.append(A.to_tensor(p).reshape(19 * 64))
    planes = np.ascontiguousarray(rng.permutation(np.stack(planes)), np.float32)
    nan_pol, nan_val = np.full((NMAX, 4096), np.nan, np.float32), np.full(NMAX, np.nan, np.float32)
    d_in, d_pol, d_val = hip.malloc(planes.nbytes), hip.malloc(nan_pol.nbytes), hip.malloc(nan_val.nbytes)
    own = hip.stream()
    try:
        for stream in (None, own):
            for n in (33, 1, 5):
                x = np.ascontiguousarray(planes[NMAX - n:])          # other rows for every n
                want_pol, want_val = net.forward(x)
                hip.copy_in(d_pol, nan_pol)
                hip.copy_in(d_val, nan_val)
                hip.copy_in(d_in, x)
                L.check(L.lib.az_net_forward_device(net._h, d_in, n, d_pol, d_val, stream))
                if stream is None:
                    L.check(L.lib.az_device_synchronize(0))
                else:
                    hip.stream_synchronize(stream)
                pol, val = hip.download(d_pol, np.zeros_like(nan_pol)), hip.download(d_val, np.zeros_like(nan_val))
                assert np.array_equal(pol[:n], want_pol) and np.array_equal(val[:n], want_val), (stream is None, n)
                assert np.all(np.abs(pol[:n].astype(np.float64).sum(1) - 1.0) <= 1e-6)
                assert np.isnan(pol[n:]).all() and np.isnan(val[n:]).all(), (stream is None, n)
    finally:
        hip.stream_destroy(own)
        for p in (d_in, d_pol, d_val):
            hip.free(p)
