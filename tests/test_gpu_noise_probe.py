"""The random streams' device functions against the oracle, bit for bit (az_noise_probe on the GPU).

The searches reach det_logf / det_expf / uniform01 / open01 / std_normal / gamma_sample only at the arguments
three values of dir_alpha produce.  az_noise_probe runs exactly those device functions -- and
dirichlet_row_block, the row k_root_noise draws -- over the sweep of tests/noisecases.py: subnormal arguments
and results, every branch threshold with its neighbours, +-0, +-inf, NaN, the extreme stream draws, eight
gamma shapes, rows that cross the 64-lane stride and fill AZ_MAX_MOVES.  Results are compared as uint32 bit
patterns, the sign of zero included; any NaN matches any NaN.  What the values must be -- float64 accuracy, the
distributions' laws -- is pinned on the oracle in tests/test_noise_laws.py; equality carries it over.

The last tests put a root whose Dirichlet row degenerates at dir_alpha = 0.03 (both gamma draws underflow to
0: the log-domain row of DESIGN 3) through the search itself."""
import numpy as np
import pytest

import azchess as A
import noisecases as N
import oracle as O
from azchess import validation as V

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", ["logf", "expf", "uniform01", "open01", "normal", "gamma"])
def test_device_function_equals_oracle(require_gpu, case):
    """one launch over the whole sweep of the function"""
    N.assert_same_bits(N.probe(case, 0), N.oracle(case), case)


@pytest.mark.parametrize("n", N.DIR_NS)
def test_device_dirichlet_rows_equal_oracle(require_gpu, n):
    """rows of n components at every alpha of the sweep, one 64-thread block each as in k_root_noise"""
    rows, fb = N.probe("dirichlet", 0, n)
    ref, rfb = N.oracle("dirichlet", n)
    N.assert_same_bits(rows, ref, "n = %d" % n)
    assert np.array_equal(fb, rfb)


def test_device_tiny_alpha_rows_equal_oracle(require_gpu):
    """alpha 0.03, n = 2, raw keys 0..19999: the degenerate rows take the log-domain path on the device as in
    the oracle, and every row is the oracle's"""
    rows, fb = N.probe("tiny", 0)
    ref, rfb = N.oracle("tiny")
    assert rfb.sum() >= 50
    assert np.array_equal(fb, rfb)
    N.assert_same_bits(rows, ref, "alpha 0.03, n = 2")


# ------------------------------------------------------------------ the degenerate row in a search
# check evasions with exactly two legal moves (the king steps aside; the checking rook is defended)
TWO_MOVE_FENS = ("8/8/8/8/8/4k3/4r3/4K3 w - - 0 1", "4k3/4R3/4K3/8/8/8/8/8 b - - 0 1")
SEED, ALPHA, EPS, SIMS = 29, 0.03, 0.25, 64
GAME_IDS = (346, 907, 1052, 1383, 0, 1)       # found by a scan of the oracle: the first four degenerate


def _degenerate(key):
    """rand_distr's arithmetic on the row's two gamma draws: sum 0 or 1/sum not finite"""
    g = np.array([O.lib().ref_gamma(ALPHA, int(k)) for k in O.component_keys(key, 2)], np.float32)
    s = np.float32(g[0] + g[1])
    with np.errstate(divide="ignore", over="ignore"):
        return bool(s == 0 or not np.isfinite(np.float32(1.0) / s))


def _roots():
    fens = [TWO_MOVE_FENS[i % 2] for i in range(len(GAME_IDS))]
    keys = [O.lib().ref_stream_key(SEED, g, 0, 0) for g in GAME_IDS]
    assert [_degenerate(k) for k in keys] == [True] * 4 + [False] * 2
    for f in TWO_MOVE_FENS:
        assert len(O.legal_indices(O.from_fen(f))) == 2
        assert sorted(A.Position.from_fen(f).legal_indices()) == sorted(O.legal_indices(O.from_fen(f)))
    return fens, keys


@pytest.mark.parametrize("fused", ["1", "0"])
def test_two_move_root_with_a_degenerate_row(require_gpu, monkeypatch, fused):
    """dir_alpha 0.03 on roots with two legal moves, under (seed, game) pairs whose row degenerates (and two
    whose row does not): the noised root priors, and the visits, improved policy, depth and most visited move
    of a 64-simulation search, are the oracle's bit for bit, through k_step and the separate kernels."""
    monkeypatch.setenv("AZ_FUSED_STEPS", fused)
    fens, keys = _roots()
    G = len(fens)
    s = A.BatchedSearch(None, games=G, sims=SIMS, noise=True, seed=SEED, cache_capacity=0, dir_alpha=ALPHA,
                        dir_eps=EPS)
    s.set_roots([[]] * G, apply_noise=True, game_ids=list(GAME_IDS), start=[A.Position.from_fen(f) for f in fens])
    trees = s.read_tree(max_depth=0)
    keep, eps = np.float32(1.0) - np.float32(EPS), np.float32(EPS)
    for g in range(G):
        pos = O.from_fen(fens[g])
        moves = O.legal_indices(pos)
        eta = O.dirichlet(ALPHA, 2, keys[g])
        assert np.all(np.isfinite(eta)) and np.all(eta >= 0) and abs(float(eta.sum()) - 1.0) < 1e-6
        want = O.synth_eval(pos)[0] * keep                       # tree.rs:282-288 as the oracle applies it
        for k, m in enumerate(moves):
            want[m] = want[m] + eps * eta[k]
        assert trees[g].moves.tolist() == moves.tolist()
        N.assert_same_bits(trees[g].policy, want, "root priors of game %d" % g)
    got = s.run()
    pv, _, _ = s.read_pv(1)
    cfg = O.make_cfg(sims=SIMS, noise=True, seed=SEED, eval_kind=0, alpha=ALPHA, eps=EPS)
    for g in range(G):
        ref = O.search_game(cfg, [], noise=True, noise_key=keys[g], start=O.from_fen(fens[g]))
        assert np.all(np.isfinite(ref[1]))
        assert np.array_equal(got[1][g].astype(np.float32), ref[0]), g
        assert np.array_equal(got[0][g], ref[1]), g
        assert got[2][g] == ref[2], g
        assert pv[g][0] == V.argmax_last(ref[0]) == V.argmax_last(got[0][g]), g
    assert s.stats()["overflow"] == 0


def test_two_move_root_degenerate_row_weighted_away(require_gpu):
    """the same roots with dir_eps = 0: the degenerate row is finite, so 0 * eta is 0 and the search is the
    noise-off search (0 * NaN poisoned both priors before)"""
    fens, keys = _roots()
    G = len(fens)
    s = A.BatchedSearch(None, games=G, sims=SIMS, noise=True, seed=SEED, cache_capacity=0, dir_alpha=ALPHA,
                        dir_eps=0.0)
    s.set_roots([[]] * G, apply_noise=True, game_ids=list(GAME_IDS), start=[A.Position.from_fen(f) for f in fens])
    trees = s.read_tree(max_depth=0)
    got = s.run()
    quiet = O.make_cfg(sims=SIMS, noise=False, seed=SEED, eval_kind=0, alpha=ALPHA, eps=0.0)
    noisy = O.make_cfg(sims=SIMS, noise=True, seed=SEED, eval_kind=0, alpha=ALPHA, eps=0.0)
    for g in range(G):
        pos = O.from_fen(fens[g])
        N.assert_same_bits(trees[g].policy, O.synth_eval(pos)[0], "root priors of game %d" % g)
        off = O.search_game(quiet, [], noise=False, start=pos)
        on = O.search_game(noisy, [], noise=True, noise_key=keys[g], start=pos)
        for ref in (off, on):
            assert np.array_equal(got[1][g].astype(np.float32), ref[0]), g
            assert np.array_equal(got[0][g], ref[1]), g
            assert got[2][g] == ref[2], g
