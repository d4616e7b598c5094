"""train(carry_games=True): one continuous SelfPlay for the whole run, iterations counted by games
finished, the games in flight carried across every weight update by SelfPlay.adopt()."""
import functools

import numpy as np
import pytest

import azchess as A
from azchess.training import _convert

pytestmark = pytest.mark.gpu

SEED = 42
ARGS = dict(blocks=2, filters=32, games=4, sims=8, min_replay=1, train_steps=1, batch_size=32, seed=SEED)
KEYS = {"iteration", "replay", "new_unique", "lr", "policy_loss", "value_loss", "selfplay_s", "train_s",
        "selfplay_games", "selfplay_sims", "games_finished", "episode_steps", "moves", "shared_replay",
        "shard_batch", "episode_steps_global"}


@functools.lru_cache(maxsize=None)
def carried_run():
    drains, adoptions = [], {}

    def log_selfplay(iteration, drained):
        assert len(drained) > 0
        drains.append((iteration, [_convert(s) for s in drained]))

    def log_adopt(iteration, flight, trainer):
        assert iteration not in adoptions
        adoptions[iteration] = (flight, trainer.params().copy())

    _, replay, hist = A.train(3, games_per_iteration=1, carry_games=True, log_selfplay=log_selfplay,
                              log_adopt=log_adopt, **ARGS)
    return drains, adoptions, len(replay), hist


def test_carried_games_are_whole_and_counted(require_gpu):
    drains, adoptions, nreplay, hist = carried_run()
    games = {}
    for _, steps in drains:
        for s in steps:
            games.setdefault(s.game_id, []).append(s)
    for gid, steps in games.items():
        assert [s.ply for s in steps] == list(range(len(steps))), gid     # every ply once, drained in order
        assert len({s.result for s in steps}) == 1 and steps[0].result != 0, gid
    assert len(hist) == 3 and sorted(adoptions) == [1, 2]
    for i, st in enumerate(hist):
        assert set(st) == KEYS | {"carried_in", "adopt_s", "selfplay_avg_batch"}
        fin = sum(len({s.game_id for s in steps}) for it, steps in drains if it == i)
        assert st["selfplay_games"] == st["games_finished"] == fin >= 1
        assert st["episode_steps"] == sum(len(steps) for it, steps in drains if it == i)
        assert st["selfplay_sims"] == st["moves"] * ARGS["sims"] and st["moves"] % ARGS["games"] == 0
        assert 0 < st["selfplay_avg_batch"] <= ARGS["games"]
        assert st["carried_in"] == (0 if i == 0 else sum(1 for _, _, ply, act, _ in adoptions[i][0] if act and ply > 0))
    assert hist[0]["adopt_s"] == 0.0 and hist[1]["carried_in"] > 0 and hist[2]["carried_in"] > 0
    assert nreplay == hist[-1]["replay"] > 0
    print("finished ids %s; carried in %s; avg batch %s"
          % (sorted(games), [st["carried_in"] for st in hist], [round(st["selfplay_avg_batch"], 2) for st in hist]))


def test_first_step_after_the_adoption_is_a_fresh_search_on_the_new_net(require_gpu):
    """every game in flight at iteration 1's adoption that finished by the end of the run: its step at
    the ply the adoption found it at has the visits of a fresh search of that history (same game id,
    noise ply) on a net built from the parameters the trainer held at the adoption."""
    drains, adoptions, _, _ = carried_run()
    flight, params = adoptions[1]
    steps = {(s.game_id, s.ply): s for _, ss in drains for s in ss}
    net = A.AlphaZero(ARGS["blocks"], ARGS["filters"], weights=params, dtype="f32")
    ref = A.BatchedSearch(net, games=1, sims=ARGS["sims"], seed=SEED, noise=True)
    checked = 0
    for _, gid, ply, active, moves in flight:
        assert active and len(moves) == ply
        s = steps.get((gid, ply))
        if s is None:
            continue                                       # still in flight when train() returned: dropped
        assert [steps[(gid, p)].action for p in range(ply)] == moves
        ref.set_roots([moves], apply_noise=True, game_ids=[gid], noise_plies=[ply])
        _, vis, dep = ref.run()
        assert s.visits == {int(a): int(vis[0][a]) for a in np.nonzero(vis[0])[0]}, (gid, ply)
        assert s.search_depth == int(dep[0])
        checked += 1
    print("checked %d of %d games in flight at the adoption" % (checked, len(flight)))
    assert checked >= 1


def test_default_path_keeps_its_keys(require_gpu):
    _, replay, hist = A.train(3, games_per_iteration=1, carry_games=False, **ARGS)
    assert len(hist) == 3 and all(set(st) == KEYS for st in hist)
    assert all(st["selfplay_games"] == ARGS["games"] == st["games_finished"] for st in hist)
    assert len(replay) == hist[-1]["replay"] > 0
