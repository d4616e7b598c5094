"""The yardstick of the leaf-parallel search tests (tests/leafpar_ref.py), checked on the CPU: with one
leaf per wave it is the oracle's search bit for bit; on a root with a single legal move it takes the
shared-leaf rule exactly as often as the definition says; and the C ABI's defaults leave the feature off."""
import ctypes

import numpy as np
import pytest

import leafpar_ref as R
import oracle as O

ONE_MOVE_FEN = "7k/p7/8/8/8/8/6q1/7K w - - 0 1"     # white's only legal move: Kh1xg2, index 3655


def random_histories(n, seed, max_len=30):
    """n histories of random legal moves that leave the game going (the oracle's rules only)"""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        g, h = O.Game(), []
        for _ in range(int(rng.integers(0, max_len))):
            idx = O.legal_indices(g.position)
            a = int(rng.choice(idx))
            if g.play_index(a) != 0:
                h = None
                break
            h.append(a)
        if h is not None and len(O.legal_indices(g.position)):
            out.append(h)
    return out


@pytest.mark.parametrize("noise", [False, True])
@pytest.mark.parametrize("sims", [16, 100])
def test_one_leaf_per_wave_is_the_oracle_search(sims, noise):
    seed = 11
    cfg = O.make_cfg(sims=sims, noise=noise, seed=seed, eval_kind=0)
    for g, h in enumerate(random_histories(6, 100 + sims + noise)):
        key = O.lib().ref_stream_key(seed, g, len(h), 0)
        rv, ri, rd, revals = O.search_game(cfg, h, noise=noise, noise_key=key)
        v, i, d, shared, evals = R.search(None, h, (sims, 1), O.synth_eval, key if noise else None)
        assert np.array_equal(v, rv), g
        assert np.array_equal(i, ri), g
        assert d == rd, g
        assert shared == 0 and evals + 1 <= revals      # the oracle also counts the root's evaluation


def test_one_move_root_is_what_the_issue_says():
    p = O.from_fen(ONE_MOVE_FEN)
    assert list(O.legal_indices(p)) == [3655]
    g = O.Game(p)
    assert g.play_index(3655) == 0                      # the game goes on


@pytest.mark.parametrize("K,shared,evals,depth", [(1, 0, 16, 4), (4, 4, 12, 4), (8, 10, 6, 2)])
def test_forced_collisions(K, shared, evals, depth):
    """A root with one legal move: the K leaves of the first wave all end on its edge, so K - 1 of them
    are shared; later waves collide wherever the tree is still narrow."""
    v, i, d, sh, ev = R.search(O.from_fen(ONE_MOVE_FEN), [], (16, K), O.synth_eval, None, c_puct=3.0)
    assert int(v.sum()) == 16 and v[3655] == 16
    assert (sh, ev, d) == (shared, evals, depth)
    assert sh + ev == 16                                # no simulation of this search ends the game


def test_wave_list_and_pair_agree():
    h = random_histories(1, 7)[0]
    a = R.search(None, h, (10, 4), O.synth_eval, None)
    b = R.search(None, h, [4, 4, 2], O.synth_eval, None)
    c = R.search(None, h, [4, 1, 4, 1], O.synth_eval, None)
    assert all(np.array_equal(x, y) for x, y in zip(a[:2], b[:2])) and a[2:] == b[2:]
    assert int(c[0].sum()) == 10


def test_chunking_a_move_changes_its_waves():
    """run_sims(5) twice (waves 4, 1, 4, 1) and run_sims(10) (waves 4, 4, 2) are different searches: on the
    roots of ply 0 of tests/test_gpu_leafpar.py's chunked-move test (games 0..3, seed 5) the restatement gives
    them different visits, which that test compares bit for bit -- it cannot pass with one schedule run as
    the other"""
    keys = [O.lib().ref_stream_key(5, g, 0, 0) for g in range(4)]
    a = [R.search(None, [], [4, 1, 4, 1], O.synth_eval, k)[0] for k in keys]
    b = [R.search(None, [], [4, 4, 2], O.synth_eval, k)[0] for k in keys]
    assert any(not np.array_equal(x, y) for x, y in zip(a, b))


def test_config_defaults():
    import azchess._lib as L
    cfg = L.AzSearchCfg()
    assert L.lib.az_search_default_cfg(ctypes.byref(cfg)) == 0
    assert cfg.leaves == 1
    assert ctypes.sizeof(L.AzSearchCfg) == 64
    assert L.AzSearchCfg.leaves.offset == 60            # the former tail padding
