"""Tree reuse on the host: the restatement (tests/treereuse_ref.py) against the oracle where nothing is
carried, its own invariants, the conditions the GPU cases of tests/test_gpu_treereuse.py rest on -- stated
from the restatement alone -- and the two C entry points.  No GPU."""
import ctypes as C
import functools

import numpy as np

import azchess._lib as L
import oracle as O
import treereuse_ref as R
from test_gpu_search import histories

SEED = 11
STEP_ROOTS, STEP_SIMS, STEP_PLIES = (6, 9), 32, 6          # the stepwise case: histories(6, 9)
DEEP_SIMS, DEEP_PLIES = 512, 4                              # the deep case: one game from the startpos


@functools.lru_cache(maxsize=None)
def step_roots():
    return histories(*STEP_ROOTS)


@functools.lru_cache(maxsize=None)
def step_reference(noise):
    """the stepwise case's restatement: per game, per ply.  Computed once, shared with the GPU tests."""
    return [R.stepwise(h, g, STEP_PLIES, STEP_SIMS, SEED if noise else None) for g, h in enumerate(step_roots())]


@functools.lru_cache(maxsize=None)
def deep_reference():
    return R.stepwise([], 0, DEEP_PLIES, DEEP_SIMS, None)


def test_first_move_is_the_oracles_search():
    """with nothing carried the restatement's move equals O.search_game, bit for bit, noise off and on"""
    for noise in (False, True):
        cfg = O.make_cfg(sims=STEP_SIMS, noise=noise, seed=SEED, eval_kind=0)
        for g, (h, plies) in enumerate(zip(step_roots(), step_reference(noise))):
            rv, ri, rd, evals = O.search_game(cfg, h, noise=noise, noise_key=R.stream_key(SEED, g, len(h)))
            first = plies[0]
            assert first["carried"] == 0 and first["kept"] == 1 and first["sims"] == STEP_SIMS
            assert np.array_equal(first["visits"], rv) and first["depth"] == rd
            assert np.array_equal(first["improved"].view(np.uint32), ri.view(np.uint32))
            assert first["evals"] + 1 == evals          # the oracle counts the root's evaluation too


def test_every_ply_tops_the_root_up_to_sims():
    for plies in step_reference(False) + step_reference(True) + [deep_reference()]:
        sims = int(plies[0]["visits"].sum())
        for rec in plies:
            assert int(rec["visits"].sum()) == sims
            assert rec["sims"] == sims - rec["carried"] >= 1
            assert rec["kept"] <= rec["carried"] + 1
            assert rec["sims"] == rec["evals"] + rec["new_terminal"] + rec["known_terminal"]
            # the move played carries its visits but the one that made its node
            assert rec["carried"] < sims


def test_conditions_of_the_gpu_cases():
    """the deep case's compactions each span more than one 64-node chunk; the 32-simulation case carries"""
    deep = deep_reference()
    assert [rec["kept"] >= 65 for rec in deep[1:]] == [True] * 3, [rec["kept"] for rec in deep]
    for noise in (False, True):
        assert sum(rec["carried"] for plies in step_reference(noise) for rec in plies) > 0


def test_selfplay_game_invariants():
    """a whole game of the self-play restatement: plies in order, one result, visits topped up"""
    game = R.selfplay_game(1, 5, 16)
    assert all(int(rec["visits"].sum()) == 16 for rec in game)
    assert game[-1]["result"] in (1, 2, 3) and len({rec["result"] for rec in game}) == 1
    assert sum(rec["carried"] for rec in game) > 0
    assert all(abs(float(rec["final_value"])) <= 1.0 for rec in game)


def test_entry_points_exist_and_refuse_a_null_handle():
    """az_search_set_tree_reuse / az_search_reuse_stats are exported, bound, and fail cleanly on NULL"""
    bound = {n for n, _, _ in L.SIGNATURES}
    assert {"az_search_set_tree_reuse", "az_search_reuse_stats"} <= bound
    assert L.lib.az_search_set_tree_reuse(None, 1) < 0
    assert b"null" in L.lib.az_last_error()
    on = C.c_int(7)
    assert L.lib.az_search_reuse_stats(None, C.byref(on), None, None, None) < 0
    assert b"null" in L.lib.az_last_error() and on.value == 7
