"""training.rs mirror of the self-play hot path: EpisodeStep, run_episode,
run_all_episodes and process_batch (src/training.rs:15-38, 294-422).

The reference runs one tokio task per game and batches leaf evaluations through an
mpsc channel; here all games of a GPU advance in lockstep inside libaz and every
simulation step evaluates all pending leaves in one batch, with nothing crossing PCIe
until a move's EpisodeSteps are drained.
"""
import ctypes as C
import time
from dataclasses import dataclass

import numpy as np

from . import _lib as L
from .chess import Position, to_tensor
from .parameters import (BATCH_SIZE, EVALUATION_GAMES, MIN_REPLAY_SIZE, NUM_EPISODES, NUM_FILTERS, NUM_RES_BLOCKS,
                         NUM_SIMULATIONS, NUM_TRAIN_STEPS, SEED, WIN_RATE_THRESHOLD)
from .tree import BatchedSearch


@dataclass
class EpisodeStep:                   # training.rs:15-20
    state: Position
    improved_policy: np.ndarray      # [4096] = visits / sum(visits)
    final_value: float
    search_depth: int
    game_id: int = 0
    ply: int = 0
    action: int = 0
    result: int = 0
    visits: dict = None


def _convert(st):
    pos = Position(L.AzPos.from_buffer_copy(st.state))
    n = st.nvis
    idx = np.frombuffer(st.vis_idx, np.uint16)[:n].astype(np.int64)
    cnt = np.frombuffer(st.vis_n, np.uint16)[:n].astype(np.float32)
    pol = np.zeros(4096, np.float32)
    tot = np.float32(cnt.sum())
    pol[idx] = cnt / tot
    return EpisodeStep(pos, pol, float(st.final_value), int(st.search_depth), int(st.game_id), int(st.ply),
                       int(st.action), int(st.result), {int(i): int(c) for i, c in zip(idx, cnt) if c})


class SelfPlay:
    """run_all_episodes engine: G game slots on one GPU.  tree_reuse=True (BatchedSearch): a game's
    re-roots keep the played move's subtree."""

    def __init__(self, model=None, games=100, device=0, continuous=False, tree_reuse=False, **cfg):
        self.search = BatchedSearch(model, games=games, device=device, continuous=continuous,
                                    tree_reuse=tree_reuse, **cfg)
        self.games = games

    @property
    def tree_reuse(self):
        return self.search.tree_reuse

    def reuse_stats(self):
        return self.search.reuse_stats()

    def reset(self):
        self.search.check(L.lib.az_selfplay_reset(self.search._h))

    def step(self):
        fin, act = C.c_int(), C.c_int()
        self.search.check(L.lib.az_selfplay_step(self.search._h, C.byref(fin), C.byref(act)))
        return fin.value, act.value

    def run_sims(self, nsims):
        """The next `nsims` simulation steps of the current move of every game; when the move
        completes, its action choice / play / re-root follow as in step().  Returns
        (finished, active, move_done); active is -1 while the move is in progress."""
        fin, act, done = C.c_int(), C.c_int(), C.c_int()
        self.search.check(L.lib.az_selfplay_run_sims(self.search._h, int(nsims), C.byref(fin), C.byref(act), C.byref(done)))
        return fin.value, act.value, bool(done.value)

    def adopt(self):
        """az_selfplay_adopt_net: between two moves, after the model was updated in place (or a
        caller-owned evaluator's model changed), carry the games in flight over to the new weights:
        every live root is evaluated again and re-noised from its (seed, game id, ply) stream, the
        start-position template of continuous mode too; histories, ids, plies and the steps recorded so
        far stay.  A no-op for a net whose generation has not moved."""
        self.search.check(L.lib.az_selfplay_adopt_net(self.search._h))

    def inflight(self):
        """The games now in the slots: [(slot, game_id, ply, active, [moves played so far])]."""
        G, h = self.games, self.search._h
        gid, ply, act = np.zeros(G, np.int32), np.zeros(G, np.int32), np.zeros(G, np.int32)
        off = np.zeros(G + 1, np.int32)
        n = L.check(L.lib.az_selfplay_inflight(h, None, None, None, None, None, 0))
        moves = np.zeros(max(n, 1), np.int32)
        L.check(L.lib.az_selfplay_inflight(h, L.i32ptr(gid), L.i32ptr(ply), L.i32ptr(act), L.i32ptr(moves),
                                           L.i32ptr(off), moves.size))
        return [(g, int(gid[g]), int(ply[g]), bool(act[g]), [int(m) for m in moves[off[g]:off[g + 1]]])
                for g in range(G)]

    def drain(self):
        return [_convert(s) for s in self.drain_raw()]

    _drain_buf = None

    def drain_raw(self):
        """EpisodeSteps of the games that ended, as the engine's az_episode_step records (what
        ReplayBuffer.add takes directly): a right-sized array per call (the 4 MB staging buffer is
        reused, so a pass that keeps its drains holds only the steps themselves)."""
        if self._drain_buf is None:
            self._drain_buf = (L.AzEpisodeStep * 4096)()
        buf, parts = self._drain_buf, []
        while True:
            n = L.check(L.lib.az_selfplay_drain(self.search._h, buf, 4096))
            if n:
                arr = (L.AzEpisodeStep * n)()
                C.memmove(arr, buf, n * C.sizeof(L.AzEpisodeStep))
                parts.append(arr)
            if n < 4096:
                break
        if len(parts) == 1:
            return parts[0]
        return (L.AzEpisodeStep * sum(len(p) for p in parts))(*[s for p in parts for s in p])


def run_all_episodes(model=None, games=100, max_moves=1000, device=0, tree_reuse=False, **cfg):
    """training.rs:340-378: play `games` games from startpos to the end; returns
    (avg_batch_size, steps) like the reference (steps of all games, game order).  avg_batch_size is network
    rows per simulation step launched; with leaves=K a step is a wave of up to K simulations per game.
    tree_reuse=True (SelfPlay): re-roots keep the played move's subtree; avg_batch_size is then rows per
    simulation run per game, the games that need fewer steps in a move counted as they ran."""
    sp = SelfPlay(model, games=games, device=device, continuous=False, tree_reuse=tree_reuse, **cfg)
    sp.reset()
    steps = []
    for _ in range(max_moves):
        _, active = sp.step()
        steps += sp.drain()
        if active == 0:
            break
    st = sp.search.stats()
    sims = max(st["sims"], 1)
    steps_per_game = sims / games                  # simulation steps launched: with leaves=K a step is a wave
    k, s = sp.search.leaves, sp.search.cfg.sims
    if k > 1:
        steps_per_game = steps_per_game * -(-s // k) / s
    avg_batch = st["evals"] / max(steps_per_game, 1)
    return avg_batch, steps


def run_episode(model=None, device=0, **cfg):
    """training.rs:294-338 for a single game."""
    return run_all_episodes(model, games=1, device=device, **cfg)[1]


def process_batch(states, model):
    """training.rs:380-422: one batched forward over the requests' positions."""
    x = np.concatenate([to_tensor(s) for s in states], 0)
    return model.forward(x)


# ---------------------------------------------------------------- train()
def get_cyclical_lr(iteration):
    """training.rs:424-441"""
    return float(L.lib.az_cyclical_lr(int(iteration)))


def comm_unique_id():
    """RCCL unique id (128 bytes) for Trainer.set_comm; create on rank 0, share over the host."""
    buf = (C.c_char * 128)()
    L.check(L.lib.az_comm_unique_id(buf, 128))
    return bytes(buf)


class Trainer:
    """The reference's training half of train() (training.rs:137-190) on one GPU: the model's
    flat parameters, the AdamW state (training.rs:63-66) and every activation of a batch live
    in HBM; one step = forward in training mode + compute_gradients + optimizer.step.
    Data-parallel over RCCL with set_comm (gradients summed over ranks before clipping)."""

    def __init__(self, blocks, filters, weights=None, max_batch=512, device=0, seed=42):
        from .agent import random_weights
        if weights is None:
            weights = random_weights(blocks, filters, seed)
        self.blocks, self.filters, self.device = blocks, filters, device
        self.n = int(L.lib.az_net_num_params(blocks, filters))
        w = np.ascontiguousarray(weights, np.float32)
        h = C.c_void_p()
        L.check(L.lib.az_trainer_create(blocks, filters, L.fptr(w), w.size, max_batch, device, C.byref(h)))
        self._h = h

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            L.lib.az_trainer_destroy(h)
            self._h = None

    @staticmethod
    def _batch(planes, tpol, tval):
        planes = np.ascontiguousarray(planes, np.float32).reshape(-1, 19 * 64)
        tpol = np.ascontiguousarray(tpol, np.float32).reshape(-1, 4096)
        tval = np.ascontiguousarray(tval, np.float32).reshape(-1)
        assert planes.shape[0] == tpol.shape[0] == tval.shape[0]
        return planes, tpol, tval

    def compute_gradients(self, planes, tpol, tval):
        planes, tpol, tval = self._batch(planes, tpol, tval)
        loss = np.zeros(2, np.float32)
        self._check(L.lib.az_trainer_compute_grads(self._h, L.fptr(planes), L.fptr(tpol), L.fptr(tval),
                                                   planes.shape[0], L.fptr(loss)))
        return float(loss[0]), float(loss[1])

    def apply(self, lr):
        self._check(L.lib.az_trainer_apply(self._h, float(lr)))

    def step(self, planes, tpol, tval, lr):
        planes, tpol, tval = self._batch(planes, tpol, tval)
        loss = np.zeros(2, np.float32)
        self._check(L.lib.az_trainer_step(self._h, L.fptr(planes), L.fptr(tpol), L.fptr(tval), planes.shape[0],
                                          float(lr), L.fptr(loss)))
        return float(loss[0]), float(loss[1])

    def compute_grads_device(self, planes, tpol, tval, batch):
        """compute_gradients on inputs already in this GPU's memory (addresses or objects with
        data_ptr(), complete when the call is made): planes [batch,19,64], policy [batch,4096],
        value [batch] f32."""
        from .memory import dev_ptr
        loss = np.zeros(2, np.float32)
        self._check(L.lib.az_trainer_compute_grads_device(self._h, dev_ptr(planes), dev_ptr(tpol), dev_ptr(tval),
                                                          int(batch), L.fptr(loss)))
        return float(loss[0]), float(loss[1])

    def step_device(self, planes, tpol, tval, batch, lr):
        """step on inputs already in this GPU's memory (as compute_grads_device): bit for bit
        step() on the same data."""
        from .memory import dev_ptr
        loss = np.zeros(2, np.float32)
        self._check(L.lib.az_trainer_step_device(self._h, dev_ptr(planes), dev_ptr(tpol), dev_ptr(tval), int(batch),
                                                 float(lr), L.fptr(loss)))
        return float(loss[0]), float(loss[1])

    def compute_grads_replay(self, replay, batch_size, seed, lo=0, hi=None):
        """compute_gradients on rows [lo, hi) (hi None: all) of replay.sample_arrays(batch_size,
        seed)'s draw, gathered on the device from a device-backed ReplayBuffer of this GPU."""
        loss = np.zeros(2, np.float32)
        self._check(L.lib.az_trainer_compute_grads_replay(self._h, replay._h, int(batch_size),
                                                          C.c_uint64(seed & (2 ** 64 - 1)), int(lo),
                                                          -1 if hi is None else int(hi), L.fptr(loss), None))
        return float(loss[0]), float(loss[1])

    def step_replay(self, replay, batch_size, seed, lr, lo=0, hi=None):
        """step on rows [lo, hi) of the same draw: bit for bit
        step(*[a[lo:hi] for a in replay.sample_arrays(batch_size, seed)[:3]], lr)."""
        loss = np.zeros(2, np.float32)
        self._check(L.lib.az_trainer_step_replay(self._h, replay._h, int(batch_size), C.c_uint64(seed & (2 ** 64 - 1)),
                                                 int(lo), -1 if hi is None else int(hi), float(lr), L.fptr(loss), None))
        return float(loss[0]), float(loss[1])

    def params(self):
        out = np.empty(self.n, np.float32)
        L.check(L.lib.az_trainer_get_params(self._h, L.fptr(out), self.n))
        return out

    def grads(self):
        out = np.empty(self.n, np.float32)
        L.check(L.lib.az_trainer_get_grads(self._h, L.fptr(out), self.n))
        return out

    def set_params(self, weights):
        """Replace the flat parameters (running statistics included) from a host array; the AdamW
        moments, the step count, the last gradients and every setting stay (az_trainer_set_params).
        Not a collective: at world > 1 every rank makes the same call."""
        w = np.ascontiguousarray(weights, np.float32).reshape(-1)
        L.check(L.lib.az_trainer_set_params(self._h, L.fptr(w), w.size))

    def set_params_device(self, weights, n=None, stream=None):
        """set_params from `n` (default: all) f32 already in this GPU's memory (an address or an object
        with data_ptr()), ordered after what `stream` holds (az_trainer_set_params_device)."""
        from .memory import dev_ptr
        L.check(L.lib.az_trainer_set_params_device(self._h, dev_ptr(weights), self.n if n is None else int(n),
                                                   dev_ptr(stream)))

    def snapshot(self):
        """new_model = model.clone() (training.rs:132): keep a copy of the current parameters in HBM
        (one per trainer; a later snapshot overwrites it)."""
        L.check(L.lib.az_trainer_snapshot(self._h))

    def restore(self):
        """Parameters <- the snapshot (a rejected candidate, training.rs:231); the AdamW state is not
        rolled back, as the reference's optimizer lives outside the loop."""
        L.check(L.lib.az_trainer_restore(self._h))

    def snapshot_params(self):
        out = np.empty(self.n, np.float32)
        L.check(L.lib.az_trainer_get_snapshot(self._h, L.fptr(out), self.n))
        return out

    @property
    def adamw_steps(self):
        """Optimizer steps applied so far (burn's AdaptiveMomentumWState::time)."""
        return int(L.check(L.lib.az_trainer_adamw_steps(self._h)))

    def relu_masks(self, batch):
        """ReLU masks of the last forward in forward order (parity tests): tower layers as
        NCHW [B, F, 8, 8], heads [B, 40, 8, 8], value hidden [B, 64]."""
        out, F = [], self.filters
        for layer in range(2 * self.blocks + 3):
            if layer <= 2 * self.blocks:
                a = np.empty(batch * 64 * F, np.float32)
            elif layer == 2 * self.blocks + 1:
                a = np.empty(batch * 64 * 64, np.float32)
            else:
                a = np.empty(batch * 64, np.float32)
            L.check(L.lib.az_trainer_relu_output(self._h, layer, L.fptr(a), a.size))
            if layer <= 2 * self.blocks:
                out.append(a.reshape(batch, 8, 8, F).transpose(0, 3, 1, 2) > 0)
            elif layer == 2 * self.blocks + 1:
                out.append(a.reshape(batch, 8, 8, 64).transpose(0, 3, 1, 2)[:, :40] > 0)
            else:
                out.append(a.reshape(batch, 64) > 0)
        return out

    _pending = None

    def _check(self, rc):
        """L.check for calls that may run the host reducer: a KeyboardInterrupt / SystemExit raised
        inside it is re-raised here, after the C call has returned its error."""
        e = self._pending[0] if self._pending else None
        if e is not None:
            self._pending[0] = None
            raise e
        return L.check(rc)

    def set_comm(self, unique_id, rank, world):
        buf = (C.c_char * 128).from_buffer_copy(unique_id)
        L.check(L.lib.az_trainer_set_comm(self._h, buf, int(rank), int(world)))

    def set_host_reducer(self, reduce, rank, world):
        """Data-parallel steps with the exchange done on the host: reduce(buf) must replace the
        float32 array buf by its element-wise sum over the `world` ranks (in place).  An exception
        inside it fails the step."""
        def fn(_ctx, ptr, n):
            try:
                reduce(np.ctypeslib.as_array(ptr, shape=(n,)))
                return 0
            except BaseException as e:       # nothing may unwind through the C frames; a
                import traceback             # KeyboardInterrupt / SystemExit is re-raised by
                traceback.print_exc()        # _check once the C call has returned (as tree.py)
                if not isinstance(e, Exception):
                    self._pending[0] = e
                return 1
        self._pending = [None]
        self._reduce_fn = L.ALLREDUCE_FN(fn)   # kept alive with the trainer
        L.check(L.lib.az_trainer_set_host_reducer(self._h, C.cast(self._reduce_fn, C.c_void_p), None, int(rank),
                                                  int(world)))

    def set_sharded(self, on=True):
        """Sharded batch (az_trainer_set_sharded): this rank's batches are its shard of one global
        batch -- the reference's single 512 step (training.rs:137-159) split over the ranks, with
        BatchNorm statistics, the BN backward and the loss over the whole global batch."""
        L.check(L.lib.az_trainer_set_sharded(self._h, int(bool(on))))

    def timing(self, reset=False):
        """(step_ms, allreduce_ms, steps): device time summed over the steps since the last reset."""
        a, b, n = C.c_double(), C.c_double(), C.c_int64()
        L.check(L.lib.az_trainer_timing(self._h, C.byref(a), C.byref(b), C.byref(n), int(reset)))
        return a.value, b.value, n.value

    def time_exchanges(self, on=True):
        """HIP events around every exchange of the following steps (for exchange_stats' time)."""
        L.check(L.lib.az_trainer_time_exchanges(self._h, int(bool(on))))

    def exchange_stats(self, reset=False):
        """(collectives, steps, exchange_ms): the data-parallel exchanges since the last reset --
        how many, over how many applied steps, and (while time_exchanges is on) their device time."""
        a, b, c = C.c_int64(), C.c_int64(), C.c_double()
        L.check(L.lib.az_trainer_exchange_stats(self._h, C.byref(a), C.byref(b), C.byref(c), int(reset)))
        return a.value, b.value, c.value

    def model(self, dtype="f32", into=None):
        """model.valid() for self-play (training.rs:83): an inference net with the current weights,
        f32 like the reference's Cuda<f32> backend (bf16 is an explicit throughput opt-in).
        into: an AlphaZero of this shape to refresh in place from the device parameters
        (AlphaZero.update_from: nothing goes to the host, its buffers and searches stay) and return."""
        from .agent import AlphaZero
        if into is not None:
            if into.dtype != dtype:
                raise ValueError("Trainer.model: into is a %s net, dtype=%r asked" % (into.dtype, dtype))
            return into.update_from(self)
        return AlphaZero(self.blocks, self.filters, weights=self.params(), dtype=dtype, device=self.device)


def sample_seed(seed, iteration, step, rank=None):
    """Seed of one training step's replay sample.  rank None: the seed every rank shares (one global
    batch drawn from the replicated buffer); else a per-rank stream."""
    s = (seed << 20) ^ (iteration << 8) ^ step
    return s if rank is None else s ^ rank << 40


def elo_seed(seed, iteration):
    """Seed of an iteration's Elo match (train(elo_evaluator=...))."""
    return (seed << 20) ^ (iteration << 8) ^ 0xE10


def gate_seed(seed, iteration):
    """Seed of an iteration's gate match (train(gate=True)).  Its low byte is 0xFE, elo_seed's 0x10 and a
    sample_seed's the step, so it differs from every elo_seed and from every sample_seed of a step < 254."""
    return (seed << 20) ^ (iteration << 8) ^ 0xFE


def gate_verdict(winrate, threshold):
    """eval.winrate >= WIN_RATE_THRESHOLD (training.rs:228): both are f32 there, so compared in float32."""
    return bool(np.float32(winrate) >= np.float32(threshold))


def agree_verdict(accepted, allgather):
    """Every rank passes its one-byte verdict through allgather(bytes) -> [bytes per rank].  Returns
    (rank 0's verdict, whether all ranks gave the same one): every rank acts on rank 0's, so the
    trainers stay identical even if the ranks' matches were to differ."""
    got = allgather(b"\x01" if accepted else b"\x00")
    votes = [bytes(b) != b"\x00" for b in got]
    return votes[0], all(v == votes[0] for v in votes)


def shard_bounds(n, rank, world):
    """This rank's contiguous rows [lo, hi) of an n-row global batch."""
    return rank * n // world, (rank + 1) * n // world


def _default_allgather(what="a shared replay buffer"):
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()):
        raise ValueError("train: world > 1 with %s needs allgather= or an initialised "
                         "torch.distributed group" % what)
    from .dist import allgather_bytes
    return allgather_bytes


def train(iterations, blocks=NUM_RES_BLOCKS, filters=NUM_FILTERS, games=NUM_EPISODES, sims=NUM_SIMULATIONS,
          min_replay=MIN_REPLAY_SIZE, train_steps=NUM_TRAIN_STEPS, batch_size=BATCH_SIZE, replay=None, trainer=None,
          device=0, seed=SEED, dtype="f32", comm=None, shard_batch=None, reducer=None, shared_replay=None,
          allgather=None, log=None, log_batch=None, device_replay=False, elo_evaluator=None,
          elo_games=EVALUATION_GAMES, elo_base=150.0, gate=False, gate_threshold=WIN_RATE_THRESHOLD,
          gate_games=EVALUATION_GAMES, log_gate=None, save_dir=None, carry_games=False, games_per_iteration=None,
          log_selfplay=None, log_adopt=None, tree_reuse=False):
    """train() (training.rs:39-275) without the TUI.  Per iteration: self-play `games` games with
    model.valid() until the replay buffer holds min_replay unique positions, then train_steps AdamW
    steps on batches of batch_size at get_cyclical_lr(iteration); the new model replaces the old one.
    The arena is off by default (SKIP_VALIDATION = true, parameters.rs:36); elo_evaluator and gate,
    below, turn on the Elo step and the model gate.

    Data parallel (comm = (unique_id, rank, world) over RCCL, or reducer = (reduce, rank, world)
    through a host callback, Trainer.set_host_reducer): every rank plays its own games (seed offset
    by rank), and by default (world > 1) the loop computes the reference's train() itself:
      * shared_replay (default on): ONE replay buffer (memory.rs:41-96), replicated -- after each
        self-play pass the ranks exchange their drained EpisodeSteps through allgather(bytes) ->
        [bytes per rank] (default: azchess.dist.allgather_bytes over torch.distributed) and every
        rank adds the union in (rank, drain) order (memory.add_from_ranks), so MIN_REPLAY_SIZE is
        tested on the global length and every rank leaves self-play together;
      * shard_batch (default on): each step is the reference's ONE batch of batch_size
        (training.rs:137-138), drawn with a seed shared by all ranks, and each rank trains its
        contiguous slice (az_trainer_set_sharded: BatchNorm statistics, BN backward and the loss
        over the whole batch).
    Labelled opt-ins: shard_batch=False trains batch_size per rank (global batch batch_size x world,
    per-rank BatchNorm, averaged gradients); shared_replay=False keeps one buffer per rank.
    log_batch(iteration, step, planes, policy, value, lo, hi): each step's drawn batch and this
    rank's rows of it.
    device_replay (opt-in): the replay buffer's payload lives in `device`'s HBM (ReplayBuffer(device=))
    and each step gathers its rows there (Trainer.step_replay) instead of sampling to the host and
    uploading; the buffer equals the host one bit for bit, so every result is the same.  A caller's
    `replay` is used as it is.
    elo_evaluator (opt-in; None: no arena, as before): an AlphaZero net to rate the model against.  Each
    iteration then ends with the reference's tail (training.rs:234-251): the model is refreshed in place
    from the trainer and compute_elo_rankings([Player.base(elo_evaluator), Player.base(model)], elo_base,
    games=elo_games, engine=True, seed=elo_seed(seed, iteration)) plays its match in the engine arena
    (validation.Arena); the iteration's entry gains `elos`, `winrate_matrix`, `arena_avg_batch` and
    `arena_s`.  Nothing else changes: the evaluator is not replaced.
    gate (opt-in; False: every trained model is kept, as SKIP_VALIDATION = true): the model gate of
    training.rs:131-132, 208-232.  Self-play runs on the incumbent net `model`, refreshed only when a
    candidate is accepted (model.generation counts the accepts).  Each iteration takes trainer.snapshot()
    before its first training step, trains as usual, brings a second net `candidate` up to date from the
    trainer and plays evaluate(Player.base(candidate), Player.base(model), games=gate_games, engine=True,
    seed=gate_seed(seed, iteration)); the candidate is kept when gate_verdict(winrate, gate_threshold).
    log_gate(iteration, candidate, model, result, accepted) runs before anything is accepted or restored.
    Accepted: model.update_from(trainer), then the Elo step (if elo_evaluator) and the checkpoints.
    Rejected: trainer.restore() -- the parameters and running statistics go back to the snapshot, the
    AdamW moments and step count stay (the reference's optimizer lives outside the loop) -- and the
    iteration has no Elo step, no checkpoint and no `elos` key.  The entry gains `accepted`,
    `gate_winrate`, `gate_p1`, `gate_draw`, `gate_p2`, `gate_avg_batch` and `gate_s`.  At world > 1 every
    rank plays the same seeded match, the verdicts go through allgather (required then) and every rank
    acts on rank 0's (agree_verdict); `gate_agree` records whether they were all equal.
    save_dir (opt-in): the checkpoints of training.rs:253-270, written by rank 0 after an accepted
    iteration (every iteration with the gate off): the model as iteration_{i}_elo_{elo:.0f}.mpk
    (iteration_{i}.mpk without an elo_evaluator), and when iteration % 3 == 0 the replay buffer as
    replay_buffer.
    carry_games (opt-in; False: the lockstep passes above, untouched): self-play games straddle the weight
    updates.  ONE SelfPlay(model, games, sims, continuous=True, seed=seed + 1000003 * rank) is created
    before the first iteration, reset once and kept for the whole run: `games` slots that are always full.
    A pass plays moves until at least games_per_iteration (default: games) more games have finished in it,
    and passes repeat until the buffer holds min_replay positions -- an iteration is counted by games
    finished, not games started.  At the top of every later iteration, after the model was refreshed in
    place, sp.adopt() carries the games in flight over to the new weights (SelfPlay.adopt: a game's plies
    before it are the old net's, every ply from it on equals a fresh search of that history on the new net;
    with the gate on and a rejected candidate the generation has not moved and it does nothing), then
    log_adopt(iteration, sp.inflight(), trainer) runs.  log_selfplay(iteration, drained) runs for every
    non-empty drain.  The entry gains `carried_in` (games in flight at the iteration's start with at least
    one move played under earlier weights; 0 in iteration 0), `adopt_s` and `selfplay_avg_batch` (network
    rows per simulation step of the iteration's self-play); `selfplay_games` is the number of games that
    finished in the iteration.  Games still in flight when train() returns are dropped: their steps reach
    neither the buffer nor the caller, and the return shape does not change.  One rank only for now
    (world > 1 raises ValueError); device_replay, elo_evaluator, gate, save_dir and dtype combine with it
    unchanged.
    tree_reuse (opt-in; False: untouched): every SelfPlay handle of the run, the carry_games one included,
    is created with tree_reuse=True (SelfPlay; weight adoption still discards the carried subtrees).  The
    entry gains `selfplay_carried_visits`, the visits the iteration's re-roots kept; `selfplay_sims` stays
    the simulations run.
    Returns (trainer, replay, per-iteration stats)."""
    from .memory import ReplayBuffer, add_from_ranks
    if comm and reducer:
        raise ValueError("train: comm (RCCL) or reducer (host), not both")
    rank, world = (comm[1], comm[2]) if comm else (reducer[1], reducer[2]) if reducer else (0, 1)
    if carry_games and world > 1:
        raise ValueError("carry_games: one rank for now")
    shard_batch = world > 1 if shard_batch is None else bool(shard_batch)
    shared_replay = world > 1 if shared_replay is None else bool(shared_replay)
    if shard_batch and batch_size < world:
        raise ValueError("shard_batch: batch_size %d is smaller than world %d" % (batch_size, world))
    if shared_replay and world > 1 and allgather is None:
        allgather = _default_allgather()
    if gate and world > 1 and allgather is None:
        allgather = _default_allgather("the model gate")
    # the largest shard a rank can get of a (possibly short) global batch
    local_batch = -(-batch_size // world) if shard_batch else batch_size
    if trainer is None:
        trainer = Trainer(blocks, filters, max_batch=local_batch, device=device, seed=seed)
        if comm:
            trainer.set_comm(*comm)
        elif reducer:
            trainer.set_host_reducer(*reducer)
    trainer.set_sharded(shard_batch)   # a caller's trainer too (its comm / reducer is the caller's)
    if replay is None:
        replay = ReplayBuffer(device=device) if device_replay else ReplayBuffer()
    elif device_replay and replay.device is None:
        raise ValueError("train: device_replay with a host-backed replay buffer")
    history = []
    model = candidate = None
    carried = None                      # carry_games: the one continuous SelfPlay of the run
    carry_target = games if games_per_iteration is None else int(games_per_iteration)
    for iteration in range(iterations):
        t0 = time.perf_counter()
        if not gate or model is None:   # gate on: the incumbent, refreshed below when a candidate is accepted
            model = trainer.model(dtype, into=model)   # created once, then refreshed in place on the device
        new_unique, plays, sims_done, games_done, steps_done, moves_done, finished = 0, 0, 0, 0, 0, 0, 0
        steps_global = 0
        carried_visits = 0
        carry = {}
        if carry_games:
            ta = time.perf_counter()
            if carried is None:
                carried = SelfPlay(model, games=games, sims=sims, device=device, continuous=True,
                                   seed=seed + 1000003 * rank, tree_reuse=tree_reuse)
                carried.reset()
                carry = {"carried_in": 0, "adopt_s": 0.0}
            else:
                carried.adopt()
                flight = carried.inflight()
                carry = {"carried_in": sum(1 for _, _, ply, active, _ in flight if active and ply > 0),
                         "adopt_s": time.perf_counter() - ta}
                if log_adopt:
                    log_adopt(iteration, flight, trainer)
            s0 = carried.search.stats()   # after the adoption: its root rows are not self-play batches
            r0 = carried.reuse_stats() if tree_reuse else None
        while carry_games:              # passes of the carried pool (the lockstep passes are the loop below)
            done = 0
            while done < carry_target:
                fin, _ = carried.step()
                done += fin
                drained = carried.drain_raw()
                if len(drained):
                    steps_done += len(drained)
                    new_unique += replay.add_many(drained)
                    if log_selfplay:
                        log_selfplay(iteration, drained)
            plays += 1
            if len(replay) >= min_replay:
                ss = carried.search.stats()
                sims_done, moves_done = ss["sims"] - s0["sims"], ss["moves"] - s0["moves"]
                finished = games_done = ss["games_finished"] - s0["games_finished"]
                carry["selfplay_avg_batch"] = (ss["evals"] - s0["evals"]) / max(sims_done / games, 1)
                if tree_reuse:
                    carried_visits += carried.reuse_stats()["carried_visits"] - r0["carried_visits"]
                break
        while not carry_games:
            sp = SelfPlay(model, games=games, sims=sims, device=device, continuous=False,
                          seed=seed + 1000003 * rank + 7919 * iteration + 104729 * plays, tree_reuse=tree_reuse)
            sp.reset()
            local = []
            while True:
                _, active = sp.step()
                drained = sp.drain_raw()
                steps_done += len(drained)
                if shared_replay and world > 1:
                    local.append(drained)
                else:
                    new_unique += replay.add_many(drained)
                if active == 0:
                    break
            if shared_replay and world > 1:
                nsteps = sum(len(d) for d in local)
                allsteps = (L.AzEpisodeStep * nsteps)()
                o = 0
                for d in local:   # this pass's drains in order, one contiguous array
                    C.memmove(C.byref(allsteps, o * C.sizeof(L.AzEpisodeStep)), d, len(d) * C.sizeof(L.AzEpisodeStep))
                    o += len(d)
                nu, added = add_from_ranks(replay, allsteps, allgather)
                new_unique += nu
                steps_global += added
            plays += 1
            ss = sp.search.stats()
            sims_done += ss["sims"]
            moves_done += ss["moves"]
            finished += ss["games_finished"]
            games_done += games
            if tree_reuse:
                carried_visits += sp.reuse_stats()["carried_visits"]
            if len(replay) >= min_replay:   # the global length when the buffer is shared
                break
        t1 = time.perf_counter()
        if gate:
            trainer.snapshot()   # new_model = model.clone(), training.rs:132
        lr = get_cyclical_lr(iteration)
        pl_sum = vl_sum = 0.0
        for b in range(train_steps):
            if device_replay:   # the same draws and rows as below, gathered in HBM into the trainer's inputs
                if shared_replay and shard_batch:
                    n, s = batch_size, sample_seed(seed, iteration, b)
                    lo, hi = shard_bounds(min(n, len(replay)), rank, world)
                    if hi <= lo:
                        raise ValueError("train: a %d-position batch leaves rank %d no rows" % (min(n, len(replay)), rank))
                else:
                    n = -(-batch_size // world) if shard_batch else batch_size
                    s = sample_seed(seed, iteration, b, rank)
                    lo, hi = 0, min(n, len(replay))
                if log_batch:
                    planes, pol, val, _ = replay.sample_arrays(n, seed=s)
                    log_batch(iteration, b, planes, pol, val, lo, hi)
                pl, vl = trainer.step_replay(replay, n, s, lr, lo, hi)
                pl_sum += pl
                vl_sum += vl
                continue
            if shared_replay and shard_batch:     # one global batch, this rank's slice
                planes, pol, val, _ = replay.sample_arrays(batch_size, seed=sample_seed(seed, iteration, b))
                lo, hi = shard_bounds(planes.shape[0], rank, world)
                if hi <= lo:
                    raise ValueError("train: a %d-position batch leaves rank %d no rows" % (planes.shape[0], rank))
            else:
                n = -(-batch_size // world) if shard_batch else batch_size
                planes, pol, val, _ = replay.sample_arrays(n, seed=sample_seed(seed, iteration, b, rank))
                lo, hi = 0, planes.shape[0]
            if log_batch:
                log_batch(iteration, b, planes, pol, val, lo, hi)
            pl, vl = trainer.step(planes[lo:hi], pol[lo:hi], val[lo:hi], lr)
            pl_sum += pl
            vl_sum += vl
        t2 = time.perf_counter()
        st = {"iteration": iteration, "replay": len(replay), "new_unique": new_unique, "lr": lr,
              "policy_loss": pl_sum / max(train_steps, 1), "value_loss": vl_sum / max(train_steps, 1),
              "selfplay_s": t1 - t0, "train_s": t2 - t1, "selfplay_games": games_done, "selfplay_sims": sims_done,
              "games_finished": finished, "episode_steps": steps_done, "moves": moves_done,
              "shared_replay": shared_replay and world > 1, "shard_batch": shard_batch,
              "episode_steps_global": steps_global if shared_replay and world > 1 else steps_done}
        st.update(carry)
        if tree_reuse:
            st["selfplay_carried_visits"] = carried_visits
        accepted, t3 = True, t2
        if gate:   # training.rs:208-232
            from .validation import Player, evaluate
            candidate = trainer.model(dtype, into=candidate)
            r = evaluate(Player.base(candidate), Player.base(model), games=gate_games, engine=True,
                         seed=gate_seed(seed, iteration), device=device)
            accepted = gate_verdict(r.winrate, gate_threshold)
            if world > 1:   # every rank played the same match; all act on rank 0's verdict
                accepted, st["gate_agree"] = agree_verdict(accepted, allgather)
            st.update(accepted=accepted, gate_winrate=r.winrate, gate_p1=r.p1_winrate, gate_draw=r.drawrate,
                      gate_p2=r.p2_winrate, gate_avg_batch=r.avg_batch_size, gate_s=time.perf_counter() - t2)
            if log_gate:
                log_gate(iteration, candidate, model, r, accepted)
            if accepted:
                model.update_from(trainer)   # model = new_model
            else:
                trainer.restore()            # the next iteration plays and trains from the old model
            t3 = time.perf_counter()
        if accepted and elo_evaluator is not None:
            from .validation import Player, compute_elo_rankings
            if not gate:
                model = trainer.model(dtype, into=model)
            avg, elos, wm = compute_elo_rankings([Player.base(elo_evaluator), Player.base(model)], elo_base,
                                                 games=elo_games, engine=True, seed=elo_seed(seed, iteration),
                                                 device=device)
            st.update(elos=[float(e) for e in elos], winrate_matrix=wm, arena_avg_batch=avg,
                      arena_s=time.perf_counter() - t3)
        if accepted and save_dir is not None and rank == 0:   # training.rs:253-270
            import os
            from .agent import save_mpk
            os.makedirs(save_dir, exist_ok=True)
            if iteration % 3 == 0:
                replay.save(os.path.join(save_dir, "replay_buffer"))
            name = "iteration_%d.mpk" % iteration
            if elo_evaluator is not None:
                name = "iteration_%d_elo_%.0f.mpk" % (iteration, st["elos"][-1])
            save_mpk(os.path.join(save_dir, name), trainer.params(), trainer.blocks, trainer.filters)
        history.append(st)
        if log:
            log(st)
    return trainer, replay, history
