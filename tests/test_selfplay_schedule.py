"""The slot schedule of a continuous self-play run, from the oracle alone: which games a run of
G slots finishes within a window of moves, given every game's length.  The GPU tests of
continuous mode (test_gpu_selfplay_continuous.py) compare finished games with the oracle's
game of the same id; this file states the conditions that make that comparison cover the
restart path (ids past the first G, one slot restarting twice, several games ending in one
move, every result), so they cannot disappear unnoticed if the oracle or the seed changes."""
import functools

import oracle as O

SIMS, SEED, SLOTS, MOVES, IDS = 16, 5, 8, 560, 24
DRAW, WHITE_WINS, BLACK_WINS = 1, 2, 3      # az_oracle.h REF_DRAW / REF_WHITE_WINS / REF_BLACK_WINS
MAX_PLIES = 398           # 200-fullmove rule: the last ply a game can reach from the startpos


@functools.lru_cache(maxsize=None)
def oracle_games(sims=SIMS, seed=SEED, ids=IDS):
    """({id: [oracle steps in ply order]}, {id: result}) of games 0..ids-1, synthetic evaluator."""
    ref, _, _ = O.selfplay(O.make_cfg(sims=sims, noise=True, seed=seed, eval_kind=0), ids)
    games = {}
    for s in ref:
        games.setdefault(s["game"], []).append(s)
    for g in games.values():
        g.sort(key=lambda s: s["ply"])
        assert [s["ply"] for s in g] == list(range(len(g)))
    return games, {k: g[0]["result"] for k, g in games.items()}


def schedule(lengths, slots, moves):
    """Replay of a continuous run: slot s starts with game s; a slot whose game ends takes the
    next unused id (ties within one move take the next ids, in slot order here: which slot gets
    which of them is not defined, the set of ids handed out at that move is).  `lengths`: plies
    of game id, indexable up to the last id handed out.  Returns (finished, per_slot, per_move):
    {id: move at which it ended} (moves count from 1), ids finished by each slot, and
    {move: [ids that ended at it]}."""
    cur = list(range(slots))
    left = [lengths[g] for g in cur]
    nxt = slots
    finished, per_slot, per_move = {}, [[] for _ in range(slots)], {}
    for m in range(1, moves + 1):
        for s in range(slots):
            left[s] -= 1
            if left[s] == 0:
                finished[cur[s]] = m
                per_slot[s].append(cur[s])
                per_move.setdefault(m, []).append(cur[s])
                cur[s] = nxt
                left[s] = lengths[nxt]
                nxt += 1
    return finished, per_slot, per_move


def check_conditions(finished, per_slot, per_move, results, lengths):
    """The conditions of the continuous-mode tests on a set of finished games (from the
    schedule, or from what a run produced)."""
    assert len(finished) >= 12
    assert sum(g >= SLOTS for g in finished) >= 5
    assert max(len(p) for p in per_slot) >= 3
    assert max(len(v) for v in per_move.values()) >= 2
    assert {results[g] for g in finished} == {DRAW, WHITE_WINS, BLACK_WINS}
    assert max(lengths[g] for g in finished) <= MAX_PLIES


def test_continuous_schedule_conditions():
    games, results = oracle_games()
    assert sorted(games) == list(range(IDS))
    lengths = {k: len(g) for k, g in games.items()}
    assert max(lengths.values()) <= MAX_PLIES
    finished, per_slot, per_move = schedule(lengths, SLOTS, MOVES)
    print("lengths", [lengths[k] for k in range(IDS)])
    print("results", [results[k] for k in range(IDS)])
    print("finished by move %d: %s" % (MOVES, sorted(finished)))
    check_conditions(finished, per_slot, per_move, results, lengths)
    # three games of this configuration end in one move: their new ids come from racing atomics
    assert max(len(v) for v in per_move.values()) >= 3
