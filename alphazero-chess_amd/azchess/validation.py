"""validation.rs / ratings.rs mirror: the evaluation arena and Elo ratings.

`evaluate(player_1, player_2)` is validation.rs:155-282 + play_evaluation_game (:284-402): G games
in lockstep, player_1 White in the even games and Black in the odd ones; an MCTS player searches
a fresh tree from the current position every move (MCTree::async_init(.., false): no noise, no
subtree reuse) -- all of that player's games to move go through ONE BatchedSearch on the GPU;
a base-model player takes the network's policy masked to the legal moves; a random player picks
uniformly from the legal-move list (under-promotions included as separate entries).
Move choice: argmax (Rust max_by: the LAST maximal index) once fullmoves > num_stochastic_moves,
else rand 0.8 WeightedIndex over the policy (float32 cumulative sums).  thread_rng is replaced by
a seeded stream per (seed, game, ply) so a match is reproducible.
`compute_elo_rankings` / `compute_elos` are ratings.rs:5-28 and :113-143 (float32, 1000
iterations of rate 8, player 0 pinned at the base Elo).
A MiniMax(n) player (chess.rs:248-322, validation.rs:113) scores all of its games to move in one
az_minimax_scores call -- the batched negamax kernels on the GPU, or the same search on the host
with device=-1 -- and takes one of the best entries with the same seeded stream; it runs no network,
so it adds nothing to num_inferences.  The human player (chess.rs:325-420, validation.rs:91-111) is
out of scope; Player.external() is its seat in the engine arena (the caller supplies the move).
`Arena` is the same match with its games in HBM (libaz az_arena_*: one az_arena_step per ply, move
generation, choice, play_move and the histories on the device); evaluate(..., engine=True) plays through
it with the same seeded uniforms and returns the same moves, results and statistics.
`Tournament` is a whole round robin in one handle (libaz az_tournament_*): every pairing of a pool advances
in lockstep and each player evaluates all of its games to move at once; evaluate_round_robin and
compute_elo_rankings(..., engine=True, tournament=True) play through it and return the pairwise matches' moves,
results and rates.
An MCTS player may bring its own search settings (Player.mcts(model, sims=, leaves=, c_puct=); libaz
az_player_search): Arena, Tournament and the host loop of evaluate all honour them, and a searching ply counts
ceil(sims / leaves) + 1 forwards.
"""
import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _lib as L
from .chess import GameState, minimax_best, minimax_scores, play_move, positions_to_array, to_tensor
from .parameters import C_PUCT, EVALUATION_GAMES, NUM_SIMULATIONS, TEMPERATURE_ANNEALING
from .tree import BatchedSearch


@dataclass
class EvaluationResult:             # validation.rs:12-19
    num_inferences: float
    avg_batch_size: float
    winrate: float
    p1_winrate: float
    p2_winrate: float
    drawrate: float


class Player:                       # validation.rs:21-27 (MctsModel, BaseModel, MiniMax, Random)
    def __init__(self, kind, model=None, depth=None, device=None, sims=None, leaves=None, c_puct=None):
        assert kind in ("mcts", "base", "random", "minimax", "external")
        self.kind, self.model, self.depth, self.device = kind, model, depth, device
        self.sims, self.leaves, self.c_puct = sims, leaves, c_puct     # an MCTS player's own search settings

    @staticmethod
    def mcts(model, sims=None, leaves=None, c_puct=None):
        """Player::MctsModel; model=None searches with libaz's synthetic evaluator (tests).  sims, leaves and
        c_puct are this player's own search settings (az_player_search); None takes the match's sims and
        c_puct, and one leaf per simulation step."""
        return Player("mcts", model, sims=sims, leaves=leaves, c_puct=c_puct)

    def search_settings(self, sims, c_puct):
        """(sims, leaves, c_puct) in effect in a match created with `sims` and `c_puct`."""
        return (self.sims or sims, self.leaves or 1, self.c_puct or c_puct)

    def search_record(self):
        """The player's az_player_search (all zero without settings of its own)."""
        return L.AzPlayerSearch(int(self.sims or 0), int(self.leaves or 0), float(self.c_puct or 0.0), 0)

    @staticmethod
    def base(model):
        return Player("base", model)

    @staticmethod
    def random():
        return Player("random")

    @staticmethod
    def minimax(depth=4, device=None):
        """Player::MiniMax(depth); device=None searches on evaluate's device, -1 on the host."""
        return Player("minimax", depth=depth, device=device)

    @staticmethod
    def external():
        """A seat whose moves the caller passes to Arena.step (the reference's Player::Human, or any
        caller-side bot); only the engine arena has it."""
        return Player("external")


def argmax_last(v):
    """Iterator::enumerate().max_by(partial_cmp): the last index among equal maxima."""
    v = np.asarray(v, np.float32)
    return int(len(v) - 1 - np.argmax(v[::-1]))


def weighted_index(w, u):
    """rand 0.8 WeightedIndex::new(w).sample(): cumulative float32 sums; x = u * total;
    the first index whose cumulative weight exceeds x."""
    w = np.asarray(w, np.float32)
    cum = np.cumsum(w, dtype=np.float32)           # sequential float32 accumulation
    total = cum[-1]
    x = np.float32(np.float32(u) * total)
    if not x < total:
        x = np.nextafter(total, np.float32(0))
    return int(np.searchsorted(cum[:-1], x, side="right"))


def choice_uniform(seed, game, ply):
    """u in [0, 1) (float32) for the move choice of (game, ply): the seeded thread_rng stand-in."""
    return np.float32(np.random.default_rng([seed, game, ply]).random(dtype=np.float32))


def choose(policy, fullmoves, num_stochastic_moves, u):
    if fullmoves > num_stochastic_moves:          # validation.rs:297 (strictly greater)
        return argmax_last(policy)
    return weighted_index(policy, u)


_KINDS = {"mcts": L.PLAYER_MCTS, "base": L.PLAYER_BASE, "minimax": L.PLAYER_MINIMAX, "random": L.PLAYER_RANDOM,
          "external": L.PLAYER_EXTERNAL}


class Arena:
    """az_arena: `games` evaluation games in HBM, player_1 White in the even games; step() plays one ply
    of every live game on the device.  A MiniMax player searches on the arena's device."""

    def __init__(self, player_1, player_2, games=EVALUATION_GAMES, sims=NUM_SIMULATIONS,
                 num_stochastic_moves=TEMPERATURE_ANNEALING, seed=0, device=0, c_puct=C_PUCT):
        self.games = games
        self._players = (player_1, player_2)          # keeps the nets alive as long as the handle

        def rec(p):
            net = p.model._h if p.kind in ("mcts", "base") and p.model is not None else None
            return L.AzArenaPlayer(_KINDS[p.kind], net, int(p.depth or 0))
        r1 = rec(player_1)
        r2 = r1 if player_1 is player_2 else rec(player_2)
        s1 = player_1.search_record()
        s2 = s1 if player_1 is player_2 else player_2.search_record()
        cfg = L.AzArenaCfg(games, sims, num_stochastic_moves, c_puct, seed)
        h = C.c_void_p()
        L.check(L.lib.az_arena_create_with(C.byref(r1), C.byref(r2), C.byref(s1), C.byref(s2), C.byref(cfg), device,
                                           C.byref(h)))
        self._h = h

    def __del__(self):
        try:
            L.lib.az_arena_destroy(self._h)
        except Exception:
            pass

    def reset(self, start=None, seed=0):
        """Every game back to live with empty histories; start: `games` Positions (or an az_pos array),
        None = the start position."""
        st = None
        if start is not None:
            arr = start if isinstance(start, np.ndarray) else positions_to_array(start)
            arr = np.ascontiguousarray(arr, L.POS_DTYPE)
            assert len(arr) == self.games
            st = arr.ctypes.data_as(C.POINTER(L.AzPos))
        L.check(L.lib.az_arena_reset(self._h, st, int(seed)))

    def step(self, u=None, actions=None):
        """One ply of every live game; u [games] float32 uniforms (None: the engine's stream), actions
        [games] for external movers.  Returns the number of games still going."""
        up = ap = None
        if u is not None:
            u = np.ascontiguousarray(u, np.float32)
            assert u.size == self.games
            up = L.fptr(u)
        if actions is not None:
            actions = np.ascontiguousarray(actions, np.int32)
            assert actions.size == self.games
            ap = L.i32ptr(actions)
        live = C.c_int()
        L.check(L.lib.az_arena_step(self._h, up, ap, C.byref(live)))
        return live.value

    def results(self):
        """(result [games]: ONGOING / DRAW / WHITE_WINS / BLACK_WINS, plies [games])"""
        res = np.zeros(self.games, np.int32)
        plies = np.zeros(self.games, np.int32)
        L.check(L.lib.az_arena_results(self._h, L.i32ptr(res), L.i32ptr(plies)))
        return res, plies

    def live(self):
        """bool [games]: the games still going, as the last step read them back (no device access)."""
        out = np.zeros(self.games, np.int32)
        L.check(L.lib.az_arena_live(self._h, L.i32ptr(out)))
        return out != 0

    def history(self, game):
        out = np.zeros(512, np.int32)
        n = L.check(L.lib.az_arena_history(self._h, int(game), L.i32ptr(out), out.size))
        return [int(a) for a in out[:n]]

    def stats(self):
        """(num_inferences, rows) since the last reset (validation.rs:209-254)."""
        a, b = C.c_double(), C.c_double()
        L.check(L.lib.az_arena_stats(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value


def tournament_matches(n_players):
    """az_tournament_pair's order (ratings.rs:10-11): [(i, j)] with j < i; players[i] is player_1 of its match."""
    n = L.check(L.lib.az_tournament_matches(int(n_players)))
    out = []
    for m in range(n):
        i, j = C.c_int(), C.c_int()
        L.check(L.lib.az_tournament_pair(int(n_players), m, C.byref(i), C.byref(j)))
        out.append((i.value, j.value))
    return out


class Tournament:
    """az_tournament: every pairing of `players` as one match of `games` games, all in HBM and advancing in
    lockstep; step() plays one ply of every live game of every match, each player evaluating all of its
    games to move at once.  Every game comes out as Arena(players[i], players[j], ...) plays it."""

    def __init__(self, players, games=EVALUATION_GAMES, sims=NUM_SIMULATIONS,
                 num_stochastic_moves=TEMPERATURE_ANNEALING, seed=0, device=0, c_puct=C_PUCT):
        self.games = games
        self._players = list(players)                 # keeps the nets alive as long as the handle
        self.matches = tournament_matches(len(self._players))
        recs = (L.AzArenaPlayer * len(self._players))()
        search = (L.AzPlayerSearch * len(self._players))()
        for k, p in enumerate(self._players):
            net = p.model._h if p.kind in ("mcts", "base") and p.model is not None else None
            recs[k] = L.AzArenaPlayer(_KINDS[p.kind], net, int(p.depth or 0))
            search[k] = p.search_record()
        cfg = L.AzArenaCfg(games, sims, num_stochastic_moves, c_puct, seed)
        h = C.c_void_p()
        L.check(L.lib.az_tournament_create_with(recs, search, len(self._players), C.byref(cfg), device, C.byref(h)))
        self._h = h

    def __del__(self):
        try:
            L.lib.az_tournament_destroy(self._h)
        except Exception:
            pass

    def reset(self, start=None, seed=0):
        """Every game of every match back to live; start: `games` Positions (or an az_pos array) -- start[g]
        opens game g of every match -- None = the start position."""
        st = None
        if start is not None:
            arr = start if isinstance(start, np.ndarray) else positions_to_array(start)
            arr = np.ascontiguousarray(arr, L.POS_DTYPE)
            assert len(arr) == self.games
            st = arr.ctypes.data_as(C.POINTER(L.AzPos))
        L.check(L.lib.az_tournament_reset(self._h, st, int(seed)))

    def step(self, u=None):
        """One ply of every live game; u [matches, games] float32 uniforms (None: the engine's stream).
        Returns the number of games still going."""
        up = None
        if u is not None:
            u = np.ascontiguousarray(u, np.float32)
            assert u.size == len(self.matches) * self.games
            up = L.fptr(u)
        live = C.c_int()
        L.check(L.lib.az_tournament_step(self._h, up, C.byref(live)))
        return live.value

    def results(self):
        """(result [matches, games]: ONGOING / DRAW / WHITE_WINS / BLACK_WINS, plies [matches, games])"""
        res = np.zeros((len(self.matches), self.games), np.int32)
        plies = np.zeros((len(self.matches), self.games), np.int32)
        L.check(L.lib.az_tournament_results(self._h, L.i32ptr(res), L.i32ptr(plies)))
        return res, plies

    def live(self):
        """bool [matches, games]: the games still going, as the last step read them back (no device access)."""
        out = np.zeros((len(self.matches), self.games), np.int32)
        L.check(L.lib.az_tournament_live(self._h, L.i32ptr(out)))
        return out != 0

    def history(self, match, game):
        out = np.zeros(512, np.int32)
        n = L.check(L.lib.az_tournament_history(self._h, int(match), int(game), L.i32ptr(out), out.size))
        return [int(a) for a in out[:n]]

    def stats(self):
        """(num_inferences, rows) of the whole tournament since the last reset."""
        a, b = C.c_double(), C.c_double()
        L.check(L.lib.az_tournament_stats(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value


def tiled_uniforms(seed, games, ply, matches):
    """[matches, games] float32: choice_uniform(seed, g, ply) depends on the game within its match only, so
    one draw per game serves every match."""
    row = np.array([choice_uniform(seed, g, ply) for g in range(games)], np.float32)
    return np.tile(row, (matches, 1))


def evaluate_round_robin(players, games=EVALUATION_GAMES, sims=NUM_SIMULATIONS,
                         num_stochastic_moves=TEMPERATURE_ANNEALING, seed=0, device=0, max_plies=1000, record=False):
    """Every pairing of `players` through one Tournament, with the per-(game, ply) uniforms of
    evaluate(engine=True).  Returns, per match in Tournament.matches order, what
    evaluate(players[i], players[j], ..., record=record) returns: the same move lists, results and rate fields.
    num_inferences and avg_batch_size are the WHOLE tournament's in every entry (a player's forward serves
    all of its matches at once, so they cannot be attributed to one match)."""
    tour = Tournament(players, games=games, sims=sims, num_stochastic_moves=num_stochastic_moves, seed=seed,
                      device=device)
    M = len(tour.matches)
    for ply in range(max_plies):
        if tour.step(tiled_uniforms(seed, games, ply, M)) == 0:
            break
    res, _ = tour.results()
    num_inferences, rows = tour.stats()
    out = []
    for m in range(M):
        result = [{L.DRAW: 0, L.WHITE_WINS: 1, L.BLACK_WINS: -1}.get(int(r)) for r in res[m]]
        hist = [tour.history(m, g) for g in range(games)] if record else None
        out.append(_evaluation_result(result, games, num_inferences, rows, hist, record))
    return out


def arena_choose(policy, fullmoves, num_stochastic_moves, u):
    """az_arena_choose: `choose` in libaz (the rule the arena kernels apply)."""
    p = np.ascontiguousarray(policy, np.float32)
    assert p.size == L.ACTION_SPACE
    return int(L.check(L.lib.az_arena_choose(L.fptr(p), int(fullmoves), int(num_stochastic_moves), C.c_float(u))))


def _evaluate_engine(player_1, player_2, G, sims, num_stochastic_moves, seed, device, max_plies, record):
    arena = Arena(player_1, player_2, games=G, sims=sims, num_stochastic_moves=num_stochastic_moves, seed=seed,
                  device=device)
    u = np.zeros(G, np.float32)
    live = np.ones(G, bool)
    for ply in range(max_plies):
        for g in np.flatnonzero(live):
            u[g] = choice_uniform(seed, int(g), ply)
        if arena.step(u) == 0:
            break
        live = arena.live()
    res, _ = arena.results()
    result = [{L.DRAW: 0, L.WHITE_WINS: 1, L.BLACK_WINS: -1}.get(int(r)) for r in res]
    num_inferences, rows = arena.stats()
    hist = [arena.history(g) for g in range(G)] if record else None
    return result, hist, num_inferences, rows


def evaluate(player_1, player_2, games=EVALUATION_GAMES, sims=NUM_SIMULATIONS,
             num_stochastic_moves=TEMPERATURE_ANNEALING, seed=0, device=0, max_plies=1000, record=False,
             engine=False):
    """validation.rs:155-282.  Returns EvaluationResult (and the games' move lists and results
    when record=True).  engine=True: the match runs through Arena (games in HBM, one az_arena_step per
    ply) with the same per-(game, ply) uniforms -- the same moves, results and statistics for MCTS,
    base-model and MiniMax players (a MiniMax player then searches on `device`; a random player draws
    with the game's uniform instead of this loop's per-ply generator)."""
    G = games
    if engine:
        result, hist, num_inferences, rows = _evaluate_engine(player_1, player_2, G, sims, num_stochastic_moves,
                                                              seed, device, max_plies, record)
        return _evaluation_result(result, G, num_inferences, rows, hist, record)
    states = [GameState() for _ in range(G)]
    hist = [[] for _ in range(G)]
    result = [None] * G                           # White's result: 1, 0, -1
    # a player moves in at most half of the games at once, or in all of them when it plays both
    # colours (player_1 is player_2)
    slots = G if player_1 is player_2 else (G + 1) // 2
    searches = {}
    for p in (player_1, player_2):
        if p.kind == "mcts" and id(p) not in searches:
            ps, pk, pc = p.search_settings(sims, C_PUCT)      # the player's own sims, leaves and c_puct
            searches[id(p)] = BatchedSearch(p.model, games=slots, device=device, sims=ps, leaves=pk, c_puct=pc,
                                            noise=False, cache_capacity=0)
    num_inferences, rows = 0, 0
    for ply in range(max_plies):
        live = [g for g in range(G) if result[g] is None]
        if not live:
            break
        white_to_move = ply % 2 == 0
        by_player = {}
        for g in live:
            white = player_1 if g % 2 == 0 else player_2
            black = player_2 if g % 2 == 0 else player_1
            p = white if white_to_move else black
            by_player.setdefault(id(p), (p, []))[1].append(g)
        actions = {}
        for p, gs in by_player.values():
            if p.kind == "random":
                rng = np.random.default_rng([seed, ply, 7])
                for g in gs:
                    legal = states[g].position.legal_indices()   # with under-promotion duplicates
                    actions[g] = int(legal[rng.integers(len(legal))])
                continue
            if p.kind == "minimax":
                entries, _ = minimax_scores([states[g].position for g in gs], p.depth,
                                            device if p.device is None else p.device)
                for g, (moves, _, scores) in zip(gs, entries):
                    actions[g] = int(moves[minimax_best(scores, choice_uniform(seed, g, ply))])
                continue
            if p.kind == "mcts":
                s = searches[id(p)]
                roots = [hist[g] for g in gs] + [hist[gs[0]]] * (slots - len(gs))   # pad with a live root
                e0 = s.stats()["evals"]
                s.set_roots(roots, apply_noise=False)
                imp, _, _ = s.run()
                pols = imp[:len(gs)]
                ps, pk, _ = p.search_settings(sims, C_PUCT)
                num_inferences += -(-ps // pk) + 1       # root batch + one batch per wave of `leaves` simulations
                rows += s.stats()["evals"] - e0
            else:
                x = np.concatenate([to_tensor(states[g].position) for g in gs], 0)
                pol, _ = p.model.forward(x)
                num_inferences += 1
                rows += len(gs)
                pols = np.zeros_like(pol)
                for k, g in enumerate(gs):
                    legal = np.unique(states[g].position.legal_indices())
                    pols[k, legal] = pol[k, legal]            # validation.rs:327-331
            for k, g in enumerate(gs):
                actions[g] = choose(pols[k], states[g].position.fullmoves, num_stochastic_moves,
                                    choice_uniform(seed, g, ply))
        for g in live:
            r = int(play_move(states[g], actions[g]))
            hist[g].append(actions[g])
            if r == 1:
                result[g] = 0
            elif r == 2:
                result[g] = 1
            elif r == 3:
                result[g] = -1
            elif r != 0:
                raise RuntimeError("player played an illegal move")
    return _evaluation_result(result, G, num_inferences, rows, hist, record)


def _evaluation_result(result, G, num_inferences, rows, hist, record):
    p1_score = [(r if g % 2 == 0 else -r) for g, r in enumerate(result) if r is not None]
    p1_wins = sum(1 for r in p1_score if r > 0)
    draws = sum(1 for r in p1_score if r == 0)
    res = EvaluationResult(float(num_inferences), rows / max(num_inferences, 1),
                           (p1_wins + draws / 2.0) / G, p1_wins / G, (G - p1_wins - draws) / G, draws / G)
    if record:
        return res, hist, result
    return res


def compute_elos(winrate_matrix, base_elo):
    """ratings.rs:113-143 in float32."""
    wm = np.asarray(winrate_matrix, np.float32)
    n = len(wm)
    f = np.float32
    elos = np.full(n, f(base_elo), np.float32)
    for _ in range(1000):
        prev = elos.copy()
        for i in range(1, n):
            actual, expected = f(0.0), f(0.0)
            for j in range(n):
                if i == j:
                    continue
                actual = f(actual + wm[i][j])
                diff = f(prev[j] - prev[i])
                expected = f(expected + f(1.0) / (f(1.0) + np.power(f(10.0), f(diff / f(400.0)))))
            elos[i] = f(elos[i] + f(8.0) * f(actual - expected))
    return elos


def compute_elo_rankings(players, base_elo=150.0, tournament=False, **kw):
    """ratings.rs:5-28: round robin, winrate matrix, Elo.  Returns (avg_batch_size, elos, matrix).
    Keywords go to evaluate (engine=True: every match through the engine arena).  tournament=True (needs
    engine=True): all matches through one Tournament (evaluate_round_robin) -- the same matrix and Elos;
    the average batch is the tournament's rows / num_inferences."""
    n = len(players)
    wm = [[0.5] * n for _ in range(n)]
    if tournament:
        kw = dict(kw)
        if not kw.pop("engine", False):
            raise ValueError("compute_elo_rankings: tournament=True plays on the device; pass engine=True")
        kw.pop("record", None)
        res = evaluate_round_robin(players, **kw)
        for (i, j), r in zip(tournament_matches(n), res):
            wm[j][i] = 1.0 - r.winrate
            wm[i][j] = r.winrate
        return res[0].avg_batch_size, compute_elos(wm, base_elo), wm
    ninf, avg = 0.0, 0.0
    for i in range(n):
        for j in range(i):
            r = evaluate(players[i], players[j], **kw)
            avg = r.avg_batch_size * r.num_inferences + avg * ninf
            ninf += r.num_inferences
            avg /= max(ninf, 1.0)
            wm[j][i] = 1.0 - r.winrate
            wm[i][j] = r.winrate
    return avg, compute_elos(wm, base_elo), wm
