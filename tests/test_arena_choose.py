"""az_arena_choose (libaz, host): the arena's move choice (validation.rs:297-308 / 337-350) against the
oracle's ref_arena_choose and validation.choose on seeded sparse policies."""
import numpy as np

import oracle as O
from azchess import validation as V

NSM = 15
U_EDGES = [np.float32(0.0), np.nextafter(np.float32(1.0), np.float32(0.0)), np.float32(1.0 - 2.0 ** -23),
           np.float32(0.5), np.float32(2.0 ** -24)]


def all_three(p, fm, u):
    a = V.arena_choose(p, fm, NSM, u)
    assert a == O.arena_choose(p, fm, NSM, u), (fm, u)
    assert a == V.choose(p, fm, NSM, u), (fm, u)
    return a


def test_random_sparse_policies():
    rng = np.random.default_rng(2025)
    for trial in range(3000):
        p = np.zeros(4096, np.float32)
        k = int(rng.integers(1, 219))
        idx = rng.choice(4096, k, replace=False)
        if trial % 3 == 0:                                  # small integers: ties at the maximum are common
            p[idx] = rng.integers(1, 4, k).astype(np.float32)
        else:
            p[idx] = rng.random(k, dtype=np.float32) + np.float32(1e-6)
        if trial % 2 == 0:
            p /= p.sum()
        if trial % 5 == 0 and k > 1:                        # an exact tie at the maximum
            p[idx[1]] = p[idx[0]] = p.max()
        fm = (NSM - 1, NSM, NSM + 1, int(rng.integers(1, 200)))[trial % 4]
        u = U_EDGES[trial % 7] if trial % 7 < len(U_EDGES) else np.float32(rng.random(dtype=np.float32))
        a = all_three(p, fm, u)
        assert p[a] > 0, trial


def test_only_the_last_entry():
    p = np.zeros(4096, np.float32)
    p[4095] = 0.75
    for fm in (1, NSM, NSM + 1, 60):
        for u in U_EDGES:
            assert all_three(p, fm, u) == 4095


def test_zero_after_one_early_entry():
    for first in (0, 1, 17):
        p = np.zeros(4096, np.float32)
        p[first] = 0.3
        for fm in (1, NSM, NSM + 1, 60):
            for u in U_EDGES:
                assert all_three(p, fm, u) == first


def test_threshold_is_strict_and_ties_take_the_last():
    p = np.zeros(4096, np.float32)
    p[[5, 900, 3000]] = [0.4, 0.4, 0.2]
    assert all_three(p, NSM + 1, np.float32(0.0)) == 900     # the last of the equal maxima
    assert all_three(p, NSM, np.float32(0.0)) == 5           # still sampled at exactly the threshold
    assert all_three(p, NSM, np.float32(0.4)) == 900
    assert all_three(p, NSM, np.float32(0.81)) == 3000


def test_engine_arena_is_opt_in():
    """The Python surface of the engine arena: present, and off unless asked for."""
    import inspect

    import azchess as A
    assert V.Player.external().kind == "external"
    assert inspect.signature(V.evaluate).parameters["engine"].default is False
    sig = inspect.signature(A.train).parameters
    assert sig["elo_evaluator"].default is None and sig["elo_games"].default == A.parameters.EVALUATION_GAMES
    assert sig["elo_base"].default == 150.0 and A.Arena is V.Arena
