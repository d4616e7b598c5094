"""Leaf-parallel search (az_search_cfg.leaves = K > 1: K leaves per game per simulation step with virtual
loss) against tests/leafpar_ref.py, the numpy-f32 restatement of its definition.  Bar: BIT-EXACT
visits, improved policies and depths, through both step forms (k_step_k; k_select_k / k_expand_k /
k_backup_k), every evaluator, the FEN cache, the self-play driver and chunked moves."""
import functools

import numpy as np
import pytest

import azchess as A
import leafpar_ref as R
import oracle as O
from test_gpu_search import histories, synthetic_process_batch

pytestmark = pytest.mark.gpu

ONE_MOVE_FEN = "7k/p7/8/8/8/8/6q1/7K w - - 0 1"     # white's only legal move: index 3655
SEED = 11


def key(seed, game, ply):
    return O.lib().ref_stream_key(seed, game, ply, 0)


def identity_holds(s, known_terminal=0):
    """every simulation is a network row, a cache hit, an expansion that found the game over, a shared leaf,
    or (known_terminal of them) a leaf selected onto an edge already known to end the game"""
    st = s.stats()
    assert st["overflow"] == 0
    assert st["sims"] == st["evals"] + st["cache_hits"] + st["terminal_leaves"] + s.shared_leaves + known_terminal, \
        (st, s.shared_leaves, known_terminal)
    return st


@functools.lru_cache(maxsize=None)
def synthetic_roots(n, hseed):
    return histories(n, hseed)


@functools.lru_cache(maxsize=None)
def synthetic_reference(n, hseed, sims, K, noise):
    """the restatement's searches of synthetic_roots(n, hseed): computed once, shared by both step forms"""
    return [R.search(None, h, (sims, K), O.synth_eval, key(SEED, g, len(h)) if noise else None)
            for g, h in enumerate(synthetic_roots(n, hseed))]


def assert_matches(out, refs):
    imp, vis, dep = out
    for g, (rv, ri, rd, _, _) in enumerate(refs):
        assert np.array_equal(vis[g].astype(np.float32), rv), g
        assert np.array_equal(imp[g], ri), g
        assert dep[g] == rd, g


# ------------------------------------------------------------------ 1. synthetic evaluator
@pytest.mark.parametrize("fused", ["1", "0"])
@pytest.mark.parametrize("noise", [False, True])
@pytest.mark.parametrize("sims,K", [(100, 2), (100, 4), (100, 8), (16, 8)])
def test_synthetic_bit_exact(require_gpu, monkeypatch, sims, K, noise, fused):
    """100 simulations: 100 mod 8 != 0, so K = 8 ends a move on a wave of 4"""
    monkeypatch.setenv("AZ_FUSED_STEPS", fused)
    hs = synthetic_roots(12, 7)
    s = A.BatchedSearch(None, games=len(hs), sims=sims, noise=noise, seed=SEED, cache_capacity=0, leaves=K)
    assert s.leaves == K
    s.set_roots(hs, apply_noise=noise)
    refs = synthetic_reference(12, 7, sims, K, noise)
    assert_matches(s.run(), refs)
    st = identity_holds(s)
    assert st["sims"] == sims * len(hs)
    assert s.shared_leaves == sum(r[3] for r in refs) and st["evals"] == sum(r[4] for r in refs)


@pytest.mark.parametrize("K", [4, 8])
def test_timing_mode_changes_no_result(require_gpu, K):
    """timing mode runs the waves that hold simulations 0, 32, 64, 96 as k_select_k / k_expand_k / k_backup_k
    between events and the others through k_step_k: the same search, four sampled steps"""
    hs = synthetic_roots(12, 7)
    s = A.BatchedSearch(None, games=len(hs), sims=100, noise=True, seed=SEED, cache_capacity=0, leaves=K)
    s.set_roots(hs, apply_noise=True)
    s.timing(reset=True, enable=True)
    assert_matches(s.run(), synthetic_reference(12, 7, 100, K, True))
    tm = s.timing(reset=False, enable=False)
    assert tm["sim_steps"] == 4 and tm["select_launches"] == 4 and 0 < tm["rows"] <= 4 * K * len(hs)
    identity_holds(s)


# ------------------------------------------------------------------ 2. one-move root
@pytest.mark.parametrize("fused", ["1", "0"])
@pytest.mark.parametrize("K", [4, 8])
def test_one_move_root_shares_leaves(require_gpu, monkeypatch, K, fused):
    """A root with one legal move: the first wave's K leaves all end on its edge, K - 1 of them shared"""
    monkeypatch.setenv("AZ_FUSED_STEPS", fused)
    sims = 16
    starts = [A.Position.from_fen(ONE_MOVE_FEN), A.Position.startpos()]
    s = A.BatchedSearch(None, games=2, sims=sims, noise=False, seed=SEED, cache_capacity=0, leaves=K)
    s.set_roots([[], []], apply_noise=False, start=starts)
    imp, vis, dep = s.run()
    refs = [R.search(O.from_fen(ONE_MOVE_FEN), [], (sims, K), O.synth_eval, None),
            R.search(None, [], (sims, K), O.synth_eval, None)]
    assert refs[0][3] >= K - 1
    assert_matches((imp, vis, dep), refs)
    assert vis[0][3655] == sims
    assert s.shared_leaves == refs[0][3] + refs[1][3]
    identity_holds(s)


# ------------------------------------------------------------------ 3. K = 1 is today's search
def test_one_leaf_is_the_current_search(require_gpu):
    hs = synthetic_roots(12, 7)
    net = A.AlphaZero(6, 64, weights=A.random_weights(6, 64, seed=42), dtype="f32")
    for model in (None, net):
        outs = []
        for kw in (dict(leaves=1), dict(leaves=0), dict()):
            s = A.BatchedSearch(model, games=len(hs), sims=24, noise=True, seed=SEED, cache_capacity=0, **kw)
            assert s.leaves == 1
            s.set_roots(hs, apply_noise=True)
            outs.append((s.run(), s.stats(), s.persistent, s.shared_leaves))
        for o in outs[1:]:
            assert all(np.array_equal(x, y) for x, y in zip(o[0], outs[0][0]))
            assert o[1:] == outs[0][1:]
        assert outs[0][3] == 0
    # the persistent per-game kernel: chosen as before at K <= 1, never at K > 1
    assert outs[0][2] is True
    s = A.BatchedSearch(net, games=len(hs), sims=24, seed=SEED, cache_capacity=0, leaves=4)
    assert s.persistent is False and A._lib.lib.az_search_persistent(s._h) == 0


# ------------------------------------------------------------------ 4. network rows beyond G
def log_evaluator(s):
    """the handle's eval log as a restatement evaluator: position -> (dense policy row, value) by fen key"""
    keys, vals, off, idx, pri = s.eval_log()
    table = {}
    for r, k in enumerate(keys):
        row = np.zeros(4096, np.float32)
        row[idx[off[r]:off[r + 1]]] = pri[off[r]:off[r + 1]]
        table[int(k)] = (row, np.float32(vals[r]))
    return lambda pos: table[int(O.fen_key(pos))]


@pytest.mark.parametrize("blocks,filters,dtype,G,sims,K", [(2, 32, "f32", 3, 32, 4), (2, 256, "f32", 1, 16, 8),
                                                           (2, 32, "bf16", 3, 32, 4)])
def test_network_rows_beyond_games(require_gpu, blocks, filters, dtype, G, sims, K):
    """More rows than games per tower launch; at 2x256 the two-board tower sees odd row counts behind its
    device-side count.  The restatement replays the handle's own evaluations (the eval log)."""
    net = A.AlphaZero(blocks, filters, weights=A.random_weights(blocks, filters, seed=42), dtype=dtype)
    hs = synthetic_roots(12, 7)[:G]
    s = A.BatchedSearch(net, games=G, sims=sims, noise=True, seed=SEED, cache_capacity=0, record_evals=True,
                        eval_log_cap=4096, leaves=K)
    s.set_roots(hs, apply_noise=True)
    out = s.run()
    ev = log_evaluator(s)
    refs = [R.search(None, h, (sims, K), ev, key(SEED, g, len(h))) for g, h in enumerate(hs)]
    assert_matches(out, refs)
    st = identity_holds(s)
    assert st["evals"] == sum(r[4] for r in refs)        # the root rows are not counted
    steps = -(-sims // K)
    assert st["evals"] > G * steps, st                 # more than G rows a step on average reached the tower


# ------------------------------------------------------------------ 5. callback evaluator
def test_callback_evaluator(require_gpu):
    hs = synthetic_roots(12, 7)[:3]
    K, sims, calls = 4, 32, []
    cb = A.BatchedSearch(None, games=3, sims=sims, noise=True, seed=SEED, cache_capacity=0, leaves=K,
                         evaluator=lambda st: synthetic_process_batch(st, calls))
    sy = A.BatchedSearch(None, games=3, sims=sims, noise=True, seed=SEED, cache_capacity=0, leaves=K)
    for s in (cb, sy):
        s.set_roots(hs, apply_noise=True)
    a, b = cb.run(), sy.run()
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    assert cb.stats() == sy.stats() and cb.shared_leaves == sy.shared_leaves
    assert 3 < max(calls[1:]) <= 3 * K, calls
    assert calls[0] == 3 and sum(calls[1:]) == cb.stats()["evals"]
    identity_holds(cb)


# ------------------------------------------------------------------ 6. FEN cache
def test_fen_cache_changes_no_result(require_gpu):
    hs = synthetic_roots(6, 9)
    outs = []
    for cap in (4096, 0):
        s = A.BatchedSearch(None, games=len(hs), sims=64, noise=True, seed=SEED, cache_capacity=cap, leaves=4)
        s.set_roots(hs, apply_noise=True)
        outs.append(s.run())
        st = identity_holds(s)
        assert cap or st["cache_hits"] == 0
        outs.append(st)
    assert all(np.array_equal(x, y) for x, y in zip(outs[0], outs[2]))
    assert outs[1]["evals"] + outs[1]["cache_hits"] == outs[3]["evals"]
    assert_matches(outs[0], synthetic_reference(6, 9, 64, 4, True))


# ------------------------------------------------------------------ 7. self-play
def check_recorded_plies(steps, seed, waves, which):
    """The plies which(n) of every recorded game of n plies against a fresh restatement search of the game's
    history so far (re-rooting keeps the child's priors and drops its subtree: traverse_new), noise from the
    game's (seed, id, ply) stream.  Returns the number of plies compared."""
    games = {}
    for st in steps:
        games.setdefault(st.game_id, {})[st.ply] = st
    n = 0
    for gid, plies in games.items():
        assert sorted(plies) == list(range(len(plies)))
        hist = [plies[p].action for p in range(len(plies))]
        for p in sorted(set(which(len(plies)))):
            st = plies[p]
            rv, _, rd, _, _ = R.search(None, hist[:p], waves, O.synth_eval, key(seed, gid, p))
            assert st.visits == {int(i): int(rv[i]) for i in np.nonzero(rv)[0]}, (gid, p)
            assert st.search_depth == rd, (gid, p)
            n += 1
    return n


def test_selfplay_records(require_gpu):
    """The driver hands out a game's plies when it ends.  The issue's call stops after 40 moves: whatever
    games ended by then are compared ply for ply.  The same games played to their ends: the first 40 plies of
    every game and its last 12 -- where the search runs into mates, stalemates and repetitions, on the
    tree and in the history -- bit for bit."""
    _, steps = A.run_all_episodes(None, games=4, sims=16, leaves=4, seed=5, max_moves=40)
    assert check_recorded_plies(steps, 5, (16, 4), lambda n: range(n)) == len(steps)
    _, steps = A.run_all_episodes(None, games=4, sims=16, leaves=4, seed=5)
    lengths = {}
    for st in steps:
        lengths[st.game_id] = max(lengths.get(st.game_id, 0), st.ply + 1)
    assert sorted(lengths) == [0, 1, 2, 3] and all(st.result in (1, 2, 3) for st in steps)
    picked = lambda n: list(range(min(n, 40))) + list(range(max(n - 12, 0), n))
    n = check_recorded_plies(steps, 5, (16, 4), picked)
    assert n == sum(len(set(picked(m))) for m in lengths.values()) and n >= 4 * 13, (n, lengths)


# ------------------------------------------------------------------ 8. chunked moves
@pytest.mark.parametrize("chunk,waves", [(5, [4, 1, 4, 1]), (10, [4, 4, 2])])
def test_chunked_moves_set_the_waves(require_gpu, chunk, waves):
    """Every az_selfplay_run_sims call starts a new wave.  A continuous handle is driven by run_sims(chunk)
    until the four games the slots started with have ended; their recorded plies 0..2 (the first three moves
    of every slot) and their last two carry the visits and depth of the restatement under that wave
    schedule.  Beside it, where a call ends mid-move, the roots read there equal the waves so far."""
    slots, sims, K, seed = 4, 10, 4, 5
    sp = A.SelfPlay(None, games=slots, sims=sims, seed=seed, continuous=True, cache_capacity=0, leaves=K)
    sp.reset()
    steps, calls = [], 0
    if chunk < sims:
        assert sp.run_sims(chunk)[2] is False
        calls = 1
        _, vis, dep = sp.search.read_roots()
        nw = next(i for i in range(1, len(waves) + 1) if sum(waves[:i]) == chunk)
        for g in range(slots):
            rv, _, rd, _, _ = R.search(None, [], waves[:nw], O.synth_eval, key(seed, g, 0))
            assert np.array_equal(vis[g].astype(np.float32), rv) and dep[g] == rd, g
    ended = set()
    while not ended >= set(range(slots)):
        assert calls < 2000, ended                       # a game is 400 plies at the most
        _, _, done = sp.run_sims(chunk)
        calls += 1
        if done:
            new = [st for st in sp.drain() if st.game_id < slots]
            steps += new
            ended |= {st.game_id for st in new}
    picked = lambda n: list(range(min(n, 3))) + list(range(max(n - 2, 0), n))
    n = check_recorded_plies(steps, seed, waves, picked)
    assert n >= slots * 3, n
    assert sp.search.stats()["sims"] == slots * chunk * calls


# ------------------------------------------------------------------ 10. the game ends inside a wave
KK_FEN = "7k/8/8/8/8/8/6q1/7K w - - 0 1"            # one legal move, Kxg2, and it leaves bare kings: a draw
BACK_RANK_FEN = "6k1/5ppp/8/8/8/8/8/R5K1 w - - 0 1"  # 17 legal moves, Ra8 mates
CORNER_FEN = "7k/5K2/8/8/8/8/8/6R1 w - - 0 1"        # 20 legal moves, Rh1 mates, others stalemate or go on
SHUFFLE = [("g1", "f3"), ("g8", "f6"), ("f3", "g1"), ("f6", "g8"), ("g1", "f3"), ("g8", "f6"), ("f3", "g1")]


@functools.lru_cache(maxsize=None)
def ending_roots():
    """(engine starts, oracle starts, histories): three positions a move away from the game's end, and the
    start position after knights out and back twice, where ...Ng8 repeats it a third time"""
    from test_oracle_search_api import move_index
    g, h = O.Game(), []
    for frm, to in SHUFFLE:
        h.append(move_index(g.position, frm, to))
        assert g.play_index(h[-1]) == 0
    fens = [KK_FEN, BACK_RANK_FEN, CORNER_FEN]
    return ([A.Position.from_fen(f) for f in fens] + [A.Position.startpos()], [O.from_fen(f) for f in fens] + [None],
            [[], [], [], h])


@functools.lru_cache(maxsize=None)
def ending_reference(sims, K):
    _, starts, hists = ending_roots()
    out = []
    for g, (st, h) in enumerate(zip(starts, hists)):
        c = {}
        out.append((R.search(st, h, (sims, K), O.synth_eval, key(SEED, g, len(h)), counts=c), c))
    return out


@pytest.mark.parametrize("fused", ["1", "0"])
@pytest.mark.parametrize("K", [4, 8])
def test_game_ends_inside_a_wave(require_gpu, monkeypatch, K, fused):
    """The rules that only fire where a game can end: a leaf whose expansion finds a mate, a stalemate, bare
    kings or a third repetition (over the leaf's own path and the history), shared leaves whose source found
    the game over, and leaves selected onto an edge already known to end it (values 0 / -1 through the
    wave's backups).  The restatement's tallies name what the engine's counters must hold."""
    monkeypatch.setenv("AZ_FUSED_STEPS", fused)
    sims = 64
    starts, _, hists = ending_roots()
    refs = ending_reference(sims, K)
    tally = {k: sum(c[k] for _, c in refs) for k in refs[0][1]}
    assert refs[0][1]["shared_terminal"] == K - 1 and refs[3][1]["new_terminal"] >= 1     # the cases are what they claim
    assert refs[1][1]["known_terminal"] > K and refs[2][1]["new_terminal"] >= 1
    s = A.BatchedSearch(None, games=len(starts), sims=sims, noise=True, seed=SEED, cache_capacity=0, leaves=K)
    s.set_roots(hists, apply_noise=True, start=list(starts))
    assert_matches(s.run(), [r for r, _ in refs])
    st = identity_holds(s, known_terminal=tally["known_terminal"])
    assert st["terminal_leaves"] == tally["new_terminal"]
    assert s.shared_leaves == sum(r[3] for r, _ in refs) and st["evals"] == sum(r[4] for r, _ in refs)


# ------------------------------------------------------------------ 9. refusals
@pytest.mark.parametrize("leaves", [9, -1])
def test_leaves_outside_the_range_are_refused(require_gpu, leaves):
    with pytest.raises(A._lib.AzError, match=r"0\.\.8"):
        A.BatchedSearch(None, games=2, sims=4, leaves=leaves)
