"""TrainPipeline: the AlphaZero loop around the batched engine -- the consumer of the hot path
(reference train_mxnet.py:38-300; SURVEY.md lists it as the "next" rows f1/f3/f4 wired together).

Same configuration keys as the reference's conf/train_config.yaml (board_width, board_height,
n_in_row, learn_rate, lr_multiplier, temp, n_playout, c_puct, buffer_size, batch_size, epochs,
kl_targ, check_freq, pure_mcts_playout_num, game_batch_num, play_batch_size, sgf_dir) plus
    concurrent_games   self-play games in flight on the GPU (default 1024)
    sgf_batches        how many leading batches replay SGF records instead of searching (the
                       reference hard-codes 4000, train_mxnet.py:270; default 0 = none)
    n_blocks, n_filter network size (the reference hard-codes 10 / 128, train_mxnet.py:79-91)
    replay             what the replay buffer stores (alphapig_amd/replay.py).  "tuples" (default): the reference's deque of 8x
                       augmented float32 tuples, filled by get_equi_data on the host.  "compact": the position codes, pi and z
                       as the exchange delivers them (1 144 B instead of 72 000 B per ply on 15x15), decoded and rotated on the
                       host for the rows a mini-batch draws.  "device": the same ring in the trainer's device memory, the
                       mini-batch gathered there by a kernel and handed to the trainer and the KL monitor without crossing
                       PCIe.  Same draws, same mini-batch bits in all three; square boards only for the last two.
    leaf_symmetry, arena_symmetry, symmetry_seed
                       the dihedral leaf symmetry ("none", "keyed", "mean8": PolicyValueNet) of the self-play evaluator and
                       of the evaluator the arena plays with, and the seed of "keyed" (default: the run's seed)
    legal_policy       False (default): the reference's policy softmax over all H*W cells.  True: over the EMPTY cells of every
                       position, in every evaluator of every rank (self-play, the trainer thread's KL monitor, the arena's
                       player: PolicyValueNet's legal_policy) and in the trainer's loss (HipTrainer's legal_policy)

One `game batch` of the reference = ONE self-play game followed by a policy update; here a batch
collects `play_batch_size` games from the engine, which keeps `concurrent_games` running so that
finished games are drawn from a continuously full GPU batch.  After every update the evaluator
is re-folded with the new weights and the engine's slots keep playing with them (their trees
were built under the previous weights -- like the reference's, whose tree is also reused across
the update that happens between two games only at game boundaries; here the switch can fall
inside a game).

Multi-GPU (BASELINE configs[4]: "competition-strength self-play for the train_mxnet.py pipeline" on 8 GPUs):
one process per GPU, `distributed=True` (default: on when alphapig_amd.dist holds a process group).  Per game batch
    every rank   self-plays its shard of the global game sequence (rank r owns games r, r + R, ...) until
                 `play_batch_size` of ITS games have finished, then joins ONE `dist.all_gather_tuples` of [codes | pi | z];
    rank 0       expands the gathered tuples (rank-major order), augments them (get_equi_data) into THE replay buffer,
                 runs `policy_update` (KL monitor and lr_multiplier live here only), saves / evaluates on schedule;
    every rank   receives rank 0's verdict (`dist.broadcast_floats`: updated?, loss, entropy, kl, lr_multiplier) and, after
                 an update, the new weights (`dist.broadcast_params`: one flat 12.7 MB RCCL broadcast, the cross-rank form of
                 the reference's predict-module re-sync, policy_value_net_mxnet.py:295-297) -> `load_device_params`
                 (device to device) and goes on playing with them.
The reference has no multi-process collector (train_mxnet.py:182-191 is commented out); the loop is its `run`
(train_mxnet.py:265-300) with collect -> all-gather -> update -> broadcast.

Two schedules (`async_update` in the configuration; default True):
  lock step    (False) the loop above, literally: every rank waits while rank 0 trains / evaluates (round 3; measured on
               one MI355X: the update is 55 % of the wall clock and self-play falls to 39 % of its rate; on N ranks every
               GPU idles through every update).
  asynchronous (True)  nobody waits for the trainer.  Self-play runs in ROUNDS of `round_seconds` wall clock (or
               `round_steps` engine steps); at the end of a round every rank hands over the games it finished since the
               last one (any number, also none) in one all-gather and receives a 10-float header from rank 0; weights
               travel only in rounds in which rank 0 has a NEW version.  On rank 0 the trainer lives in its own thread
               with its own HIP stream, its own evaluator handle (KL monitor, arena) and its own HipTrainer: it takes
               the gathered game batches from a queue, puts them into the replay buffer, runs `policy_update` -- one per
               game batch like the reference, never more; batches that arrive while an update runs are merged into the
               next one and counted as `updates_skipped` -- saves / evaluates on the reference's schedule and publishes a
               snapshot of the weights, which the next round broadcasts.  The SGF bootstrap batches (`sgf_batches`,
               train_mxnet.py:270-271) run on the trainer thread first, one record + one update per batch, while the ranks
               already self-play; they count as game batches.  Staleness bound: a rank plays with weights that
               are at most (one round + one policy_update + one broadcast) older than the trainer's; the switch can fall
               inside a game, as in lock step.  `max_update_share` < 1 makes the trainer pause after an update so that it
               is busy at most that share of the time (on ONE GPU self-play and training share the device: the
               reference's one-update-per-game rule costs 0.36 - 0.55 of it; see profiles/r04_train_loop_15x15.log).

Checkpoints (`checkpoint_every` game batches, default 0 = never; `resume=` of the constructor; alphapig_amd/checkpoint.py has
the file layout).  Lock step: saved after batch i when (i + 1) % checkpoint_every == 0, and a resumed run() starts at the
saved batch index with the trainer's weights installed in the evaluator the way an update installs them -- the run that was
never stopped, bit for bit.  Asynchronous: the cut is a round boundary; when the collected games cross a multiple of
checkpoint_every * play_batch_size rank 0 sets the header's tenth field, every rank writes its self-play part at that
boundary, and rank 0 queues a marker behind that round's games; its trainer thread, on reaching the marker, writes the
trainer, the buffer and the schedule and completes the directory.  The buffer then holds exactly the games handed over
before the cut; self-play does not wait.  Consistent, and as timing-dependent as the schedule itself.

Every weight set that leaves a trainer for an evaluator goes through trainer_weights / load_weights / sync_weights
(alphapig_amd/train.py): device to device where both sides can, else through the host.  The optional keys, their checks and
what a resumed run must share with the checkpoint's are one table, _CONF_KEYS.
"""
import logging
import os
import queue
import random
import threading
import time

import numpy as np

from . import checkpoint, dist, sgf
from .arena import Arena, win_ratio
from .augment import get_equi_data
from .game import Board, Game
from .policy_value_net import EvaluatorError, PolicyValueNet, check_leaf_symmetry
from .selfplay import SelfPlayEngine
from .train import FRAMED_SIDES, check_ema_decay, load_weights, policy_update, sync_weights, trainer_weights

_logger = logging.getLogger(__name__)


class ReplayBuffer(object):
    """The reference's `deque(maxlen=buffer_size)` of (state, pi, z) tuples (train_mxnet.py:59) with O(1) random access:
    `random.sample` on the deque costs O(buffer) per mini-batch (the reference's buffer holds 2 198 800 entries), a list
    used as a ring does not.  Index 0 is the oldest entry, as in the deque."""

    def __init__(self, maxlen):
        self.maxlen = int(maxlen)
        self._items = []
        self._head = 0                   # position of the oldest entry once the ring is full

    def __len__(self):
        return len(self._items)

    def __getitem__(self, i):
        n = len(self._items)
        if i < 0:
            i += n
        if not 0 <= i < n:
            raise IndexError(i)
        return self._items[(self._head + i) % n] if n == self.maxlen else self._items[i]

    def append(self, x):
        if len(self._items) < self.maxlen:
            self._items.append(x)
        else:
            self._items[self._head] = x
            self._head = (self._head + 1) % self.maxlen

    def extend(self, xs):
        for x in xs:
            self.append(x)

    def __iter__(self):
        for i in range(len(self._items)):
            yield self[i]

    def sample(self, rng, k):
        """`rng.sample(list(buffer), k)` -- the same draws from the same generator state -- without the copy."""
        return [self[j] for j in rng.sample(range(len(self._items)), k)]

    def state(self):
        """The entries, oldest first, stacked: {"meta": maxlen and count, "states", "pis", "zs"} (9 000 B per entry on 15x15
        where the code buffers of alphapig_amd/replay.py keep 143)."""
        items = list(self)
        out = {"meta": {"maxlen": self.maxlen, "n": len(items)}}
        for j, name in enumerate(("states", "pis", "zs")):
            out[name] = np.stack([np.asarray(x[j]) for x in items]) if items else np.zeros(0, np.float32)
        return out

    def load_state(self, state):
        if int(state["meta"]["maxlen"]) != self.maxlen:
            raise ValueError("this replay state was taken with maxlen=%r, the buffer has maxlen=%r" %
                             (state["meta"]["maxlen"], self.maxlen))
        n = int(state["meta"]["n"])
        if n > self.maxlen or (n and not len(state["states"]) == len(state["pis"]) == len(state["zs"]) == n):
            raise ValueError("this replay state does not hold the %d entries it announces" % n)
        self._items = [(state["states"][i], state["pis"][i], state["zs"][i]) for i in range(n)]
        self._head = 0


def _one_of(key, *allowed):
    def check(value):
        if value not in allowed:
            raise ValueError("%s must be %s or %r, not %r" % (key, ", ".join(repr(a) for a in allowed[:-1]), allowed[-1], value))
        return value
    return check


def _clip_norm(value):
    if value is None:
        return None
    if not (np.isfinite(float(value)) and float(value) > 0):
        raise ValueError("clip_norm must be None or a finite positive number, not %r" % (value,))
    return float(value)


_SKIP = object()        # last column: a checkpoint without the key is not compared on it
# The optional configuration keys: (name = attribute, default, check or conversion, a resumed run must share it, what a
# checkpoint from before the key counts as).  TrainPipeline.__init__ reads them in this order (the first bad value raises),
# _conf_match holds the shared ones, _resume compares them.  Required keys a resumed run must share: _SHARED_KEYS.
_CONF_KEYS = (
    ("async_update", True, bool, False, None),
    ("round_seconds", 0.5, float, False, None),
    ("round_steps", None, None, False, None),
    ("max_update_share", 1.0, float, False, None),
    # exclusive_updates: rank 0's self-play loop starts no new round while its trainer thread is inside a policy_update
    # (the in-flight forwards finish): 45 ms updates instead of 130, 277 k leaf evaluations/s against 305 k interleaved
    # (profiles/r06_train_loop_exclusive.log / _interleaved.log) -- for jobs that want the shortest
    # update latency.
    ("exclusive_updates", False, bool, False, None),
    # train_arith: the trainer's trunk arithmetic (HipTrainer's trunk_arith)
    ("train_arith", "f32", _one_of("train_arith", "f32", "f16x2"), False, None),
    # act_scale: the static activation exponents of the self-play evaluator's f16x2 trunk kernel (PolicyValueNet.
    # calibrate_trunk).  "off": untouched, all 0.  "auto": the evaluators lower their exponents when a forward overflows,
    # and the self-play evaluator is calibrated on its most recent code batch after every weight installation.
    ("act_scale", "off", _one_of("act_scale", "off", "auto"), False, None),
    # leaf_symmetry / arena_symmetry / symmetry_seed (module docstring).  An evaluator that is asked for a mode other than
    # "none" needs set_leaf_symmetry (ValueError otherwise); with "none" it is never called.  Where the arena plays with the
    # self-play evaluator itself (lock step), it holds arena_symmetry for the arena's duration only.  state.json holds the
    # three beside "conf", and only when one is not "none" (_SYMMETRY_KEYS).
    ("leaf_symmetry", "none", lambda v: check_leaf_symmetry(v, "leaf_symmetry"), True, "none"),
    ("arena_symmetry", "none", lambda v: check_leaf_symmetry(v, "arena_symmetry"), True, "none"),
    ("symmetry_seed", None, int, True, _SKIP),
    # replay: what the replay buffer stores (module docstring)
    ("replay", "tuples", _one_of("replay", "tuples", "compact", "device"), True, None),
    # train_framed: HipTrainer's `framed` -- the training step on the framed boards (6x6, 7x7, 9x9, 11x11 .. 14x14: the 15x15
    # trunk kernels, the board mask in the BatchNorm passes).  On such a board it goes with the tuple buffer and the f32
    # trainer only; 15x15 and 8x8 train as they always did, whatever the key says.
    ("train_framed", False, bool, True, False),
    # legal_policy (module docstring): an evaluator that was passed in is switched over (set_legal_policy: ValueError if it
    # has none); with the key absent nothing is called and the run is what it was.
    ("legal_policy", False, bool, True, False),
    # step_guard / clip_norm: HipTrainer's guarded optimiser step -- a step whose gradients or losses are not finite is
    # skipped on the device instead of reaching the weights, the moments and, through them, every self-play evaluator and
    # the next checkpoint; clip_norm (a finite positive number; implies the guard) clips the global gradient norm.  The
    # history record counts skipped and clipped steps; a skipped one is logged.
    ("step_guard", False, bool, True, False),
    ("clip_norm", None, _clip_norm, True, None),
    # ema_decay / ema_warmup: HipTrainer's averaged weights.  With ema_decay set, everything that leaves the trainer for
    # play -- the weights the self-play evaluators receive, the arena's, the saved .model files -- is the exponential
    # moving average of the weights; the raw weights go on being trained, and every forward of the KL monitor runs on them.
    # With None, none of that code runs.
    ("ema_decay", None, check_ema_decay, True, None),
    ("ema_warmup", True, bool, True, _SKIP),      # (from before the averaged weights: ema_decay, compared first, was off)
    # checkpoints (module docstring).  checkpoint_every: game batches between two of them, 0 = never; checkpoint_keep: how
    # many complete ones stay on disk; checkpoint_selfplay: "games" saves the games in flight with their trees, "none"
    # abandons them (the game sequence and the finished games nobody took are kept either way); checkpoint_buffer: whether
    # the replay buffer travels (default: the code buffers do, the 9 000 B tuples do not)
    ("checkpoint_every", 0, lambda v: int(v or 0), False, None),
    ("checkpoint_keep", 2, int, False, None),
    ("checkpoint_selfplay", "games", _one_of("checkpoint_selfplay", "games", "none"), False, None),
)
_SHARED_KEYS = ("board_width", "board_height", "n_in_row", "n_blocks", "n_filter", "batch_size", "buffer_size", "concurrent_games")
_SYMMETRY_KEYS = ("leaf_symmetry", "arena_symmetry", "symmetry_seed")


class TrainPipeline(object):
    def __init__(self, conf, init_model=None, policy_value_net=None, device=0, seed=0, distributed=None, trainer=None,
                 eval_net=None, resume=None):
        """policy_value_net: an evaluator to use instead of building the HIP PolicyValueNet (needs evaluate_codes, params /
        set_params; policy_value for the KL monitor on rank 0).  trainer: an object with HipTrainer's interface
        (train_step, get_params; optionally sync_evaluator) to use instead of creating a HipTrainer -- the CPU tests pass
        stand-ins for both.  eval_net (asynchronous schedule, rank 0): the trainer thread's own evaluator for the KL
        monitor, checkpoints and the arena; default: a second HIP PolicyValueNet, or `policy_value_net` itself when one
        was passed in.  distributed: None = on iff alphapig_amd.dist holds a process group.
        resume: the directory of a checkpoint (save_checkpoint; conf key checkpoint_every) written by a pipeline of the same
        board, net, batch_size, buffer_size, replay, train_framed, legal_policy, step_guard, clip_norm, concurrent_games and
        world size:
        run() goes on where that one stood."""
        conf = {"symmetry_seed": seed, **conf}          # (the seed of "keyed": by default the run's)
        for name, default, check, _, _ in _CONF_KEYS:
            value = conf.get(name, default)
            setattr(self, name, value if check is None else check(value))
        self.step_guard = self.step_guard or self.clip_norm is not None
        # uniform_trunk: the evaluators this pipeline builds itself run batches of <= 32 boards on the small-batch f16x2
        # kernel, so that a game's bits do not depend on how many games share a forward (PolicyValueNet's uniform_trunk).  The
        # trainer's internal evaluator is not concerned.
        self.uniform_trunk = bool(conf.get("uniform_trunk", False))
        self.checkpoint_buffer =bool(conf.get("checkpoint_buffer", self.replay != "tuples"))
        # what the keys ask of each other and of the objects passed in
        for net, mode, key in ((policy_value_net, self.leaf_symmetry, "leaf_symmetry"),
                               (eval_net if eval_net is not None else policy_value_net, self.arena_symmetry, "arena_symmetry")):
            if net is not None and mode != "none" and not hasattr(net, "set_leaf_symmetry"):
                raise ValueError("%s=%r needs an evaluator with set_leaf_symmetry; %r has none" % (key, mode, net))
        if (self.async_update and self.arena_symmetry != self.leaf_symmetry and policy_value_net is not None and
                trainer is not None and (eval_net is None or eval_net is policy_value_net)):
            raise ValueError("arena_symmetry=%r differs from leaf_symmetry=%r, and the asynchronous schedule's arena would play "
                             "with the self-play evaluator while it is in use: pass eval_net" %
                             (self.arena_symmetry, self.leaf_symmetry))
        if self.legal_policy:
            for net, what in ((policy_value_net, "policy_value_net"), (eval_net, "eval_net")):
                if net is not None and not hasattr(net, "set_legal_policy"):
                    raise ValueError("legal_policy=True needs an evaluator with set_legal_policy; %s %r has none" % (what, net))
            if trainer is not None and not getattr(trainer, "legal_policy", True):
                raise ValueError("legal_policy=True, but the trainer %r was built with legal_policy=False" % (trainer,))
        if self.train_framed:
            bw, bh = int(conf["board_width"]), int(conf["board_height"])
            if bw == bh and bw in FRAMED_SIDES:
                if self.replay != "tuples":
                    raise ValueError("train_framed on a %dx%d board takes replay='tuples', not %r: the code replay buffers' "
                                     "framed form does not exist" % (bw, bh, self.replay))
                if self.train_arith != "f32":
                    raise ValueError("train_framed on a %dx%d board takes train_arith='f32', not %r: the f16x2 trunk's "
                                     "statistics epilogue and scales see off-board cells" % (bw, bh, self.train_arith))
        if self.ema_decay is not None and trainer is not None:
            # (a HipTrainer built without ema_decay has both names: ema_p is None and ema_params() raises)
            keeps = (getattr(trainer, "ema_p", None) is not None or
                     (not hasattr(trainer, "ema_p") and callable(getattr(trainer, "ema_params", None))))
            if not keeps or (hasattr(trainer, "ema_decay") and trainer.ema_decay is None):
                raise ValueError("ema_decay=%r needs a trainer that keeps averaged weights (ema_p / ema_params()); %r has "
                                 "none" % (self.ema_decay, trainer))
            own_kl_net = self.async_update and eval_net is not None and eval_net is not policy_value_net
            if not own_kl_net and not hasattr(trainer, "policy_value"):
                raise ValueError("ema_decay=%r: the self-play evaluator holds the averaged weights, so the KL monitor needs "
                                 "a trainer with policy_value (its own evaluator on the raw weights), or eval_net on the "
                                 "asynchronous schedule; %r has none" % (self.ema_decay, trainer))
        self._kl_net_averaged = False           # the trainer thread's evaluator holds the average (an arena or a save put it there)
        if self.replay == "device":
            import torch
            if not torch.cuda.is_available():
                raise RuntimeError("replay='device' keeps the replay buffer in GPU memory and there is no GPU "
                                   "(replay='compact' keeps the same codes on the host)")
            if trainer is not None and not hasattr(trainer, "upload"):
                raise RuntimeError("replay='device' hands the trainer mini-batches in GPU memory; the trainer passed in has "
                                   "no upload(), so it does not take device batches (replay='compact' stays on the host)")
        self._gpu_gate = threading.Event()
        self._gpu_gate.set()
        self._custom_net = policy_value_net is not None
        self._eval_net = eval_net
        self._device = device
        self.distributed = dist.is_active() if distributed is None else bool(distributed)
        self.rank, self.world = dist.rank_world() if self.distributed else (0, 1)
        # what a resumed run must share with the run that wrote the checkpoint (_main_state, _resume)
        self._conf_match = {k: conf.get(k) for k in _SHARED_KEYS}
        self._conf_match.update({name: getattr(self, name) for name, _, _, shared, _ in _CONF_KEYS if shared}, world=self.world)
        self._trainer_override = trainer
        self._seed = seed
        self._train_steps = 0
        self.board_width, self.board_height = conf["board_width"], conf["board_height"]
        self.n_in_row = conf["n_in_row"]
        self.learn_rate, self.lr_multiplier = conf["learn_rate"], conf.get("lr_multiplier", 1.0)
        self.temp, self.n_playout, self.c_puct = conf["temp"], conf["n_playout"], conf["c_puct"]
        self.batch_size = conf["batch_size"]
        self.data_buffer = ReplayBuffer(conf["buffer_size"])
        self.play_batch_size = conf.get("play_batch_size", 1)
        self.epochs, self.kl_targ = conf["epochs"], conf["kl_targ"]
        self.check_freq, self.game_batch_num = conf["check_freq"], conf["game_batch_num"]
        self.pure_mcts_playout_num = conf["pure_mcts_playout_num"]
        self.eval_games = conf.get("eval_games", 10)
        self.best_win_ratio = 0.0
        self.sgf_batches = conf.get("sgf_batches", 0)
        self._sgf_home = conf.get("sgf_dir")
        self._training_data = []
        if self.sgf_batches and self._sgf_home and os.path.isdir(self._sgf_home):
            self._training_data = sgf.get_files_as_list(self._sgf_home)
            random.shuffle(self._training_data)
        self.model_dir = conf.get("model_dir", "./logs")
        self.checkpoint_dir = conf.get("checkpoint_dir") or os.path.join(self.model_dir, "checkpoints")
        self.board = Board(width=self.board_width, height=self.board_height, n_in_row=self.n_in_row)
        self.game = Game(self.board)
        concurrent = conf.get("concurrent_games", 1024)
        self.policy_value_net = policy_value_net or PolicyValueNet(
            self.board_width, self.board_height, max(self.batch_size, (concurrent + 1) // 2),
            n_blocks=conf.get("n_blocks", 10), n_filter=conf.get("n_filter", 128), model_params=init_model,
            device=device, seed=seed, uniform_trunk=self.uniform_trunk, leaf_symmetry=self.leaf_symmetry,
            symmetry_seed=self.symmetry_seed, legal_policy=self.legal_policy)
        if self.legal_policy:
            for net in (policy_value_net, eval_net):
                if net is not None:
                    net.set_legal_policy(True)
        if self._custom_net and self.leaf_symmetry != "none":
            self.policy_value_net.set_leaf_symmetry(self.leaf_symmetry, self.symmetry_seed)
        self.engine = SelfPlayEngine(self.policy_value_net, self.board_width, self.board_height, self.n_in_row,
                                     n_games=concurrent, n_playout=self.n_playout, c_puct=self.c_puct,
                                     temp=self.temp, base_seed=seed, pipeline=2,
                                     forced_opening=(self.board_width == 15 and self.board_height == 15),
                                     index_offset=self.rank, index_stride=self.world)
        if self.act_scale == "auto":
            self.policy_value_net.set_act_scale_auto(True)
            if eval_net is not None and eval_net is not self.policy_value_net:
                eval_net.set_act_scale_auto(True)
        self.keep_replica_buffers = bool(conf.get("replica_buffers", False))    # every rank keeps the replay buffer (host RAM x world)
        if self.replay != "tuples":
            from . import replay
            c_in = int(getattr(self.policy_value_net, "channelnum", 9))
            if self.replay == "device" and (self.rank == 0 or self.keep_replica_buffers):
                self.data_buffer = replay.DeviceReplayBuffer(conf["buffer_size"], self.board_height, self.board_width, c_in,
                                                             device=device)
            else:       # (also the ranks that never fill theirs: untouched zero pages)
                self.data_buffer = replay.CompactReplayBuffer(conf["buffer_size"], self.board_height, self.board_width, c_in)
        self._taken = 0
        self._rng = random.Random(seed)
        self.episode_len = 0
        self.history = []
        # asynchronous schedule
        self.weights_version = 0
        self.weight_broadcasts = 0
        self.update_intervals = []              # rank 0: (start, end) wall clock of every policy_update (time.time())
        self.round_log = []                     # every rank: (time.time(), leaf evaluations so far) at the end of each round
        self.updates_done = self.updates_skipped = 0
        self._train_q = None
        self._fresh = None
        self._lock = threading.Lock()
        self._trainer_error = None
        self._sgf_done = threading.Event()     # asynchronous schedule: set by rank 0's trainer thread behind the SGF bootstrap
        self._last = (0.0, 0.0, 0.0)
        self._trainer_thread = self._async_trainer = self._async_trainer_state = None
        self._own_eval_net = False              # the trainer thread built its evaluator itself: close() closes it
        self._template = None                   # _param_template
        self._held = None                       # device tensors the self-play evaluator may still be packing from
        self.last_gathered = self.last_monitors = None
        self._batches_done = 0                # lock step: the loop index run() starts at
        self._eval_overflows0 = 0               # the self-play evaluator's overflow count before a resume
        self.trainer_history = []
        self._games_collected = 0
        self._round = 0
        self._async_resume = None               # asynchronous schedule: what the trainer thread picks up (resume=)
        self.checkpoint_log = []                # one record per part written: (part, seconds, bytes)
        if resume is not None:
            self._resume(resume)

    # ---- data collection -----------------------------------------------------------------
    def collect_selfplay_data_ai(self, n_games=1):
        """train_mxnet.py:170-180, batched: take the next n finished games from the engine (of THIS rank's shard; with
        several ranks the batch is the rank-major concatenation of every rank's n games)."""
        while len(self.engine.finished) < n_games:           # completion order, like a game queue
            self.engine.run_steps(16)
        eps = self.engine.finished[:n_games]
        del self.engine.finished[:n_games]
        self._taken += n_games
        self.episode_len = int(np.mean([len(e.moves) for e in eps]))
        block = self._episodes_block(eps, exchange=self.distributed)
        if self.distributed:
            block = dist.all_gather_tuples(*block, consumer=None if self.keep_replica_buffers else 0)   # THE exchange of the round (RCCL all-gather)
            self.last_gathered = dist.last_gather_total
            if self.rank != 0 and not self.keep_replica_buffers:
                return
        self._buffer_block(*block)

    def _episodes_block(self, eps, exchange=True):
        """Finished episodes as one block (codes, pis, zs), for none the empty block; exchange: pis and zs as float32, the
        form that travels between ranks and to the trainer thread (a single rank's lock step buffers them as they are)."""
        if not eps:
            return (np.zeros((0, self.engine.pool.code_stride), np.uint8),
                    np.zeros((0, self.board_width * self.board_height), np.float32), np.zeros(0, np.float32))
        codes, pis, zs = (np.concatenate([getattr(e, k) for e in eps]) for k in ("codes", "pis", "zs"))
        return (codes, pis.astype(np.float32), zs.astype(np.float32)) if exchange else (codes, pis, zs)

    def _buffer_block(self, codes, pis, zs):
        """A block into the replay buffer: the codes as they are, or their planes, 8x augmented (get_equi_data)"""
        if self.replay != "tuples":
            self.data_buffer.extend_codes(codes, pis, zs)
        else:
            states = self.engine.pool.codes_to_planes(codes, 9)
            self.data_buffer.extend(get_equi_data(list(zip(states, pis, zs)), self.board_height, self.board_width))

    def collect_selfplay_data(self, training_index):
        """train_mxnet.py:137-154: SGF replay phase."""
        name = self._training_data[training_index % len(self._training_data)]
        warning, winner, data = self.game.start_self_play(_NoPlayer(), sgf_home=self._sgf_home, file_name=name)
        if warning:
            _logger.error("WARNING: bad SGF record %s", name)
            return
        data = list(data)
        self.episode_len = len(data)
        if self.replay != "tuples":             # game records yield planes: stored as the codes that reproduce them
            if data:
                self.data_buffer.extend_planes(np.stack([np.asarray(d[0], dtype=np.float32) for d in data]),
                                               np.stack([np.asarray(d[1]).reshape(-1) for d in data]), [d[2] for d in data])
            return
        self.data_buffer.extend(get_equi_data(data, self.board_height, self.board_width))

    # ---- update / evaluation ---------------------------------------------------------------
    def _trainer(self):
        net = self.policy_value_net
        if self._trainer_override is not None:
            return self._trainer_override
        if getattr(net, "_trainer", None) is None:
            if self.ema_decay is not None and self._train_steps > 0:
                # none of this pipeline's own paths drops the trainer; an outside set_params on the evaluator does.  With
                # ema_decay the evaluator holds the AVERAGE, so the new trainer's raw weights start from it
                _logger.warning("the trainer was dropped (set_params on the self-play evaluator?): with ema_decay=%r the new "
                                "trainer starts its raw weights, its moments and its average from the averaged weights "
                                "the evaluator holds", self.ema_decay)
            # a re-created trainer (set_params dropped the old one) continues the dropout mask sequence instead of replaying it
            net._trainer = self._new_trainer(net, dropout_step0=self._train_steps)
        return net._trainer

    def _new_trainer(self, net, dropout_step0=0):
        """A HipTrainer on evaluator `net`'s weights with this pipeline's training keys"""
        from .train import HipTrainer           # (looked up now: the tests put stand-ins there)
        return HipTrainer(net.params(), net.net_kind, net._n_blocks, batch_size=self.batch_size, device_index=net._device,
                          seed=self._seed, dropout_step0=dropout_step0, trunk_arith=self.train_arith,
                          framed=self.train_framed, step_guard=self.step_guard, clip_norm=self.clip_norm,
                          ema_decay=self.ema_decay, ema_warmup=self.ema_warmup, legal_policy=self.legal_policy)

    # ---- the averaged weights (conf ema_decay): what plays is the average, what the KL monitor reads is the raw weights
    def _average_for_play(self, trainer, net):
        """Before an arena or a save on the trainer thread's evaluator: it gets the averaged weights, and the next update
        puts the raw ones back before its first forward (policy_update).  The self-play evaluator already holds the average
        (every installation carries it)."""
        if self.ema_decay is None or net is self.policy_value_net:
            return
        sync_weights(trainer, net, averaged=True, keep_trainer=True)
        self._kl_net_averaged = True

    def _note_overflows(self, rec, trainer):
        """train_arith f16x2: the update record carries the trainer's count of steps repeated on the exact kernels;
        step_guard / clip_norm: its counts of skipped and clipped steps so far and the last step's gradient norm"""
        if self.train_arith == "f16x2":
            rec["trunk_overflows"] = int(getattr(trainer, "trunk_overflows", 0))
        if self.step_guard:
            rec["skipped_steps"] = int(getattr(trainer, "skipped_steps", 0))
            rec["clipped_steps"] = int(getattr(trainer, "clipped_steps", 0))
            # (a skipped step's norm is NaN or inf: None in the record, which travels into a checkpoint's state.json --
            # json.dump would write the tokens NaN / Infinity, which strict JSON readers refuse)
            norm = getattr(trainer, "last_grad_norm", None)
            rec["grad_norm"] = float(norm) if norm is not None and np.isfinite(norm) else None
        if self.ema_decay is not None:      # averaging steps applied so far (a skipped optimiser step is none)
            rec["ema_updates"] = int(getattr(trainer, "ema_updates", 0))

    def _note_act_scale(self, rec):
        """Every round / batch record carries the self-play evaluator's count of forwards repeated on the exact kernel
        (evaluators without such a count: left out); act_scale "auto": its current activation exponents too."""
        net = self.policy_value_net
        if hasattr(net, "trunk_overflows"):
            rec["eval_trunk_overflows"] = self._eval_overflows0 + int(net.trunk_overflows())
        if self.act_scale == "auto":
            rec["act_exponents"] = [int(a) for a in net.trunk_act_exponents()]

    def _calibrate_after_install(self):
        """act_scale "auto": new weights move the activation ranges -- calibrate the self-play evaluator on the most
        recent self-play code batch (none yet: skipped; the overflow response still holds)."""
        if self.act_scale != "auto":
            return
        codes = getattr(self.engine, "last_codes", None)
        if codes is None or not len(codes):
            return
        cap = int(getattr(self.policy_value_net, "batchsize", len(codes)))
        self.policy_value_net.calibrate_trunk(codes=codes[:cap])

    def policy_update(self, trainer=None, kl_net=None):
        """train_mxnet.py:194-240 (rank 0 of a multi-rank run; see `_exchange_update` / `_trainer_main`).  Lock step: the
        self-play evaluator itself supplies the old / new predictions of the KL monitor (re-folded per epoch);
        asynchronous: the trainer thread's own evaluator `kl_net` does, and the self-play evaluator is left alone.
        ema_decay: every forward of the KL monitor runs on the RAW weights.  Where the monitor's evaluator would be the
        self-play evaluator (lock step), which holds the average, the trainer's own evaluator takes its place; the trainer
        thread's `kl_net` gets the raw weights back first when an arena or a save left the average in it.  The caller
        installs the average in the self-play evaluator."""
        mini = self.data_buffer.sample(self._rng, self.batch_size)
        net = self.policy_value_net if kl_net is None else kl_net
        trainer = self._trainer() if trainer is None else trainer
        t_before = getattr(trainer, "t", 0)
        mon = {}
        evaluator = None if self.ema_decay is not None and net is self.policy_value_net else _KeepTrainer(net)
        if evaluator is not None and self._kl_net_averaged:     # (only ema_decay sets it)
            sync_weights(trainer, net, keep_trainer=True)
            self._kl_net_averaged = False
        loss, entropy, kl, self.lr_multiplier = policy_update(trainer, mini, self.learn_rate, self.lr_multiplier,
                                                              self.epochs, self.kl_targ, evaluator=evaluator, monitors=mon)
        self._train_steps += max(0, getattr(trainer, "t", 0) - t_before)
        self.last_monitors = mon                          # train_mxnet.py:222-239: the value head's explained variance
        _logger.info("kl:%.4f lr:%.1e lr_multiplier:%.3f loss:%.4f entropy:%.4f explained_var_old:%.3f explained_var_new:%.3f",
                     kl, mon["learn_rate"], self.lr_multiplier, loss, entropy, mon["explained_var_old"], mon["explained_var_new"])
        if mon.get("skipped_steps"):        # a guarded trainer refused steps: the mini-batch or the activations were not finite
            _logger.warning("policy_update: %d optimiser step(s) skipped (%s), %d so far; grad_norm %r", mon["skipped_steps"],
                            getattr(trainer, "last_skip_reason", None), int(getattr(trainer, "skipped_steps", 0)),
                            mon.get("grad_norm"))
        return loss, entropy, kl

    def _exchange_update(self, rec):
        """The update step of one game batch across ranks: rank 0 decides and trains, everybody learns the outcome and, if
        the weights changed, receives them (module docstring).  Single rank: just the update."""
        do = self.rank == 0 and len(self.data_buffer) > self.batch_size
        if not self.distributed:
            if do:
                rec["loss"], rec["entropy"], rec["kl"] = self.policy_update()
                self._note_overflows(rec, self._trainer())
                if self.ema_decay is not None:      # the games that follow are played by the average
                    sync_weights(self._trainer(), self.policy_value_net, averaged=True, keep_trainer=True)
            return
        head = [0.0, 0.0, 0.0, 0.0, self.lr_multiplier]
        if do:
            loss, entropy, kl = self.policy_update()
            head = [1.0, loss, entropy, kl, self.lr_multiplier]
            self._note_overflows(rec, self._trainer())
        head = dist.broadcast_floats(head, src=0)
        if head[0] == 0.0:
            return
        rec["loss"], rec["entropy"], rec["kl"] = head[1], head[2], head[3]
        rec["lr_multiplier"] = head[4]          # informational on ranks > 0: the adaptive state lives on rank 0
        net = self.policy_value_net
        if self.rank == 0:
            src = trainer_weights(self._trainer(), self.ema_decay is not None)
            if self.ema_decay is not None:
                # the broadcast carries the average, and rank 0's own evaluator, which the KL monitor no longer touches, gets it too
                sync_weights(self._trainer(), net, averaged=True, keep_trainer=True)
        else:
            src = self._param_template()
        got = dist.broadcast_params({k: src[k] for k in sorted(src)}, src=0)
        if self.rank != 0:      # (the evaluator packs from device tensors asynchronously: _held keeps them alive)
            self._held = load_weights(net, got, keep_trainer=False) or self._held
        self.weight_broadcasts += 1

    def _param_template(self):
        """Names and shapes of the parameter set (ranks > 0 never build a trainer; values are overwritten by the broadcast)."""
        if self._template is None:
            self._template = {k: np.zeros(v.shape, np.float32) for k, v in self.policy_value_net.params().items()}
        return self._template

    def policy_evaluate(self, n_games=None, net=None):
        """train_mxnet.py:242-263: win ratio of the current net against pure MCTS."""
        net = net or self.policy_value_net
        # the arena's evaluator holds arena_symmetry while the arena plays, and what it held before afterwards (the self-play
        # evaluator of the lock-step schedule: between two run_steps calls no slot is in flight)
        held = getattr(net, "leaf_symmetry", "none")
        switch = held != self.arena_symmetry
        if switch and not hasattr(net, "set_leaf_symmetry"):
            raise ValueError("arena_symmetry=%r needs an evaluator with set_leaf_symmetry; %r has none" % (self.arena_symmetry, net))
        if switch:
            net.set_leaf_symmetry(self.arena_symmetry, self.symmetry_seed)
        try:
            res = Arena(net, self.board_width, self.board_height, self.n_in_row,
                        n_playout=self.n_playout, c_puct=self.c_puct, pure_mcts_playout_num=self.pure_mcts_playout_num,
                        base_seed=len(self.history)).play(n_games or self.eval_games)
        finally:
            if switch:
                net.set_leaf_symmetry(held, self.symmetry_seed)
        return win_ratio(res)

    def run(self):
        """train_mxnet.py:265-300; with several ranks every rank runs this loop (module docstring)."""
        if self.async_update:
            return self._run_async()
        lead = self.rank == 0
        for i in range(self._batches_done, self.game_batch_num):
            if i < self.sgf_batches and self._training_data:
                if lead:                                    # game records are rank 0's (lock step: the other ranks wait in the next collective)
                    self.collect_selfplay_data(i)
            else:
                self.collect_selfplay_data_ai(self.play_batch_size)
            rec = {"batch": i + 1, "episode_len": self.episode_len, "buffer": len(self.data_buffer)}
            self._exchange_update(rec)
            if "loss" in rec:                          # the evaluator holds new weights
                self._calibrate_after_install()
            self._note_act_scale(rec)
            if lead:            # (the self-play evaluator holds what plays, the average included: no trainer is passed)
                self._schedule_after_batch(i, rec, self.policy_value_net)
            self.history.append(rec)
            _logger.info("batch %s", rec)
            self._batches_done = i + 1
            if self.checkpoint_every and (i + 1) % self.checkpoint_every == 0:
                self.save_checkpoint(os.path.join(self.checkpoint_dir, "ckpt_%08d" % (i + 1)))
                if lead:
                    checkpoint.prune(self.checkpoint_dir, self.checkpoint_keep)
        return self.history

    # ---- checkpoints (alphapig_amd/checkpoint.py holds the file layout) ------------------------------------------------
    def _timed_part(self, directory, part, state):
        """Write one part; state: the part's state, or a function that returns it (its time counts)"""
        t0 = time.perf_counter()
        nbytes = checkpoint.write_part(directory, part, state() if callable(state) else state)
        self.checkpoint_log.append((part, time.perf_counter() - t0, nbytes))

    def _write_selfplay_part(self, directory):
        """This rank's engine, between two run_steps calls (the caller's thread is the one that drives the engine)"""
        self._timed_part(directory, "selfplay_rank%d" % self.rank,
                         lambda: self.engine.state(games=self.checkpoint_selfplay == "games"))

    def _write_trainer_parts(self, directory, trainer):
        """Rank 0: the trainer (or, before the first update, the evaluator's weights) and the replay buffer"""
        if trainer is not None:
            if not hasattr(trainer, "state"):
                raise RuntimeError("a checkpoint needs a trainer with state() / load_state(); %r has none" % (trainer,))
            self._timed_part(directory, "trainer", trainer.state())
        else:
            self._timed_part(directory, "weights", dict(self.policy_value_net.params(), meta={}))
        if self.checkpoint_buffer:
            self._timed_part(directory, "buffer", self.data_buffer.state())

    def _schedule_state(self):
        """The values the training side owns (lock step: the one thread; asynchronous: the trainer thread)"""
        return {"lr_multiplier": self.lr_multiplier, "best_win_ratio": self.best_win_ratio,
                "pure_mcts_playout_num": self.pure_mcts_playout_num, "train_steps": self._train_steps,
                "rng": checkpoint.rng_to_json(self._rng), "updates_done": self.updates_done,
                "updates_skipped": self.updates_skipped, "trainer_history": list(self.trainer_history),
                "last": list(self._last), "with_buffer": self.checkpoint_buffer}

    def _main_state(self):
        """The values the self-play side owns, and the configuration a resumed run must share"""
        net = self.policy_value_net
        conf = {k: v for k, v in self._conf_match.items() if k not in _SYMMETRY_KEYS}
        out = {"format": checkpoint.FORMAT, "conf": conf, "async_update": self.async_update,
               "next_batch": self._batches_done, "taken": self._taken, "episode_len": self.episode_len,
               "weights_version": self.weights_version, "games_collected": self._games_collected, "round": self._round,
               "training_data": list(self._training_data), "history": list(self.history),
               "checkpoint_selfplay": self.checkpoint_selfplay,
               "eval_trunk_overflows": self._eval_overflows0 + (int(net.trunk_overflows()) if hasattr(net, "trunk_overflows") else 0)}
        if self.leaf_symmetry != "none" or self.arena_symmetry != "none":     # (a run without them writes what it always wrote)
            out.update({k: self._conf_match[k] for k in _SYMMETRY_KEYS})
        if hasattr(net, "trunk_act_exponents"):
            try:
                out["act_exponents"] = [int(a) for a in net.trunk_act_exponents()]
            except EvaluatorError:          # (the 8x8 kernels and the other arithmetics have no such exponents)
                pass
        return out

    def save_checkpoint(self, path):
        """Write everything a later TrainPipeline(conf, resume=path) needs to go on from here: legal between two game
        batches of the lock-step schedule (run() calls it every `checkpoint_every` batches; the asynchronous schedule
        writes its checkpoints itself, at a round boundary).  With several ranks every rank calls it, with the same path on
        a file system all of them see: each writes its own self-play part, rank 0 the rest."""
        lead = self.rank == 0
        tmp = checkpoint.tmp_path(path)
        if lead:
            checkpoint.begin(path)
        if self.distributed:
            dist.barrier()
        self._write_selfplay_part(tmp)
        if self.distributed:
            dist.barrier()
        if not lead:
            return path
        missing = [r for r in range(self.world) if not checkpoint.has_part(tmp, "selfplay_rank%d" % r)]
        if missing:
            raise RuntimeError("checkpoint %s: no self-play part of rank(s) %s -- every rank must write into the same "
                               "directory (conf checkpoint_dir on a file system all ranks see)" % (path, missing))
        trainer = self._trainer_override
        if trainer is None:
            trainer = getattr(self.policy_value_net, "_trainer", None)
        self._write_trainer_parts(tmp, trainer)
        state = self._main_state()
        state.update(self._schedule_state())
        checkpoint.finish(path, state)
        _logger.info("checkpoint %s", path)
        return path

    def _resume(self, path):
        state = checkpoint.read_state(path)
        absent = {name: value for name, _, _, _, value in _CONF_KEYS}     # what a checkpoint from before a key counts as
        for k, mine in self._conf_match.items():
            theirs = (state if k in _SYMMETRY_KEYS else state["conf"]).get(k, absent.get(k))
            if theirs is not _SKIP and theirs != mine:
                raise ValueError("the checkpoint %s was written with %s=%r, this pipeline has %s=%r" %
                                 (path, k, theirs, k, mine))
        if bool(state["async_update"]) != self.async_update:
            raise ValueError("the checkpoint %s was written with async_update=%r" % (path, state["async_update"]))
        part = "selfplay_rank%d" % self.rank
        if not checkpoint.has_part(path, part):
            raise ValueError("the checkpoint %s has no part %s" % (path, part))
        self.engine.load_state(checkpoint.read_part(path, part))
        self.lr_multiplier = state["lr_multiplier"]
        self.best_win_ratio = state["best_win_ratio"]
        self.pure_mcts_playout_num = state["pure_mcts_playout_num"]
        self._train_steps = state["train_steps"]
        checkpoint.rng_from_json(self._rng, state["rng"])
        self.updates_done, self.updates_skipped = state["updates_done"], state["updates_skipped"]
        self._last = tuple(state["last"])
        self._batches_done = state["next_batch"]
        self._taken, self.episode_len = state["taken"], state["episode_len"]
        self.weights_version = state["weights_version"]
        self._games_collected, self._round = state["games_collected"], state["round"]
        self._training_data = list(state["training_data"])
        self.history = list(state["history"])
        self.trainer_history = list(state["trainer_history"])
        self._eval_overflows0 = int(state.get("eval_trunk_overflows", 0))
        net = self.policy_value_net
        has_buffer = self.rank == 0 or self.keep_replica_buffers
        if has_buffer and checkpoint.has_part(path, "buffer"):
            self.data_buffer.load_state(checkpoint.read_part(path, "buffer"))
        elif has_buffer:
            _logger.info("the checkpoint %s holds no replay buffer: the resumed run starts with an empty buffer", path)
        # the weights: the trainer's, installed in the self-play evaluator the way an update installs them
        tstate = checkpoint.read_part(path, "trainer") if checkpoint.has_part(path, "trainer") else None
        if tstate is None:
            w = checkpoint.read_part(path, "weights")
            load_weights(net, {k: v for k, v in w.items() if k != "meta"}, keep_trainer=True)
        else:
            weights = {k[2:]: v for k, v in tstate.items() if k.startswith("p/")}
            if self.ema_decay is not None and any(k.startswith("e/") for k in tstate):
                weights = {k[2:]: v for k, v in tstate.items() if k.startswith("e/")}       # what plays is the average
            if self.rank == 0 and (self._trainer_override is not None or not self.async_update):
                tr = self._trainer()
                if not hasattr(tr, "load_state"):
                    raise RuntimeError("resume needs a trainer with state() / load_state(); %r has none" % (tr,))
                tr.load_state(tstate)
                sync_weights(tr, net, averaged=self.ema_decay is not None, keep_trainer=True)
            else:
                if self.rank == 0:
                    self._async_trainer_state = tstate          # the trainer thread builds its trainer, then loads this
                if hasattr(net, "load_device_params") and hasattr(net, "_device"):
                    # through device tensors where the evaluator folds and packs on the device: what a broadcast update does
                    import torch
                    dev = torch.device("cuda", int(net._device))
                    weights = {k: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).to(dev) for k, v in weights.items()}
                    torch.cuda.synchronize(dev)
                self._held = load_weights(net, weights, keep_trainer=True) or self._held
        if "act_exponents" in state and hasattr(net, "set_trunk_act_exponents") and any(state["act_exponents"]):
            net.set_trunk_act_exponents(state["act_exponents"])
        self._async_resume = {"games_recv": state.get("games_recv", 0), "batches_done": state.get("trainer_batches_done", 0)}
        if self.ema_decay is not None:
            # the asynchronous schedule's trainer thread builds its evaluator from the self-play evaluator's weights, which are
            # now the average (and one passed in holds whatever it held): the first update puts the raw weights into it
            # before its first forward, as after an arena or a save
            self._kl_net_averaged = True
        if self.async_update:
            self.weights_version = max(self.weights_version, int(self.updates_done))   # (versions count updates; the evaluator holds the trainer's)
        _logger.info("resumed from %s: next batch %d, %d games taken so far", path, self._batches_done, self._taken)

    # ---- the asynchronous schedule (module docstring) ---------------------------------------------
    def _play_round(self):
        if self.round_steps:
            self.engine.run_steps(int(self.round_steps))
            return
        t_end = time.perf_counter() + self.round_seconds
        while True:
            self.engine.run_steps(8)
            if time.perf_counter() >= t_end:
                return

    def _schedule_after_batch(self, i, rec, net, first=None, trainer=None):
        """The reference's per-batch schedule behind the update (train_mxnet.py:283-298): checkpoint every 50 batches,
        arena every check_freq.  i = 0-based game-batch index.  `first` (asynchronous schedule): the update covered the
        game batches first ... i (a cluster of games finished in one round); the weights are the same for all of them, so a
        checkpoint / an arena evaluation runs ONCE if the range crosses a multiple, not once per skipped index.
        ema_decay: the saved model and the arena's player are the averaged weights of `trainer`."""
        lo = i if first is None else first
        crosses = lambda m: (i + 1) // m > lo // m          # some k in (lo, i + 1] is a multiple of m
        if trainer is not None and (crosses(50) or crosses(self.check_freq)):
            self._average_for_play(trainer, net)
        if crosses(50):
            os.makedirs(self.model_dir, exist_ok=True)
            net.save_model(os.path.join(self.model_dir, "current_policy.model"))
        if crosses(self.check_freq):
            rec["win_ratio"] = wr = self.policy_evaluate(net=net)
            if wr > self.best_win_ratio:
                self.best_win_ratio = wr
                os.makedirs(self.model_dir, exist_ok=True)
                net.save_model(os.path.join(self.model_dir, "best_policy_%s.model" % i))
                if self.best_win_ratio >= 0.98 and self.pure_mcts_playout_num < 8000:
                    self.pure_mcts_playout_num += 1000
                    self.best_win_ratio = 0.0

    def _trainer_main(self):
        """Rank 0's trainer thread: replay buffer, policy_update, checkpoints, arena -- never on the self-play path."""
        try:
            import contextlib
            ctx = contextlib.nullcontext()
            net = self.policy_value_net
            kl_net = self._eval_net
            trainer = self._trainer_override
            if trainer is None:
                import torch
                stream = torch.cuda.Stream(device=net._device)
                ctx = torch.cuda.stream(stream)      # this thread's kernels: a stream of their own, beside the self-play stream
                if kl_net is None:
                    kl_net = self._eval_net = PolicyValueNet(
                        self.board_width, self.board_height, self.batch_size, n_blocks=net._n_blocks,
                        n_filter=net._n_filter, model_params=net.params(), net_kind=net.net_kind, device=net._device,
                        uniform_trunk=self.uniform_trunk, legal_policy=self.legal_policy)
                    self._own_eval_net = True
                    if self.act_scale == "auto":
                        kl_net.set_act_scale_auto(True)
            elif kl_net is None:
                kl_net = self._eval_net = net
            with ctx:
                if trainer is None:
                    trainer = self._new_trainer(net)
                self._async_trainer = trainer
                if self._async_trainer_state is not None:       # resume=: the trainer this thread built continues the saved one
                    trainer.load_state(self._async_trainer_state)
                    self._async_trainer_state = None
                resumed = self._async_resume or {}
                games_recv = int(resumed.get("games_recv", 0))
                busy_until = 0.0
                stop = False
                # SGF bootstrap (train_mxnet.py:270-271: the first batches replay game records instead of searching):
                # game batches 0 ... n_sgf - 1, one record + one policy_update each, here on the trainer thread.  Self-play
                # starts from the net these batches trained (train_mxnet.py:268-272): every rank HOLDS in _run_async until
                # `_sgf_done` is set, so no game of the untrained net enters the buffer or counts toward the budget.
                n_sgf = self._sgf_phase_batches()
                for i in range(min(n_sgf, int(resumed.get("batches_done", 0))), n_sgf):
                    before = len(self.data_buffer)
                    self.collect_selfplay_data(i)
                    # (the record's own length: self.episode_len belongs to the main thread once self-play runs)
                    ep_len = (len(self.data_buffer) - before) // 8 if len(self.data_buffer) > before else 0
                    rec = {"batch": i + 1, "sgf": True, "episode_len": ep_len or self.episode_len, "buffer": len(self.data_buffer)}
                    if len(self.data_buffer) == before:
                        rec["skipped"] = True                            # an unreadable record: nothing joined the buffer
                    if len(self.data_buffer) > self.batch_size:
                        self._async_update(trainer, kl_net, rec)
                    self._schedule_after_batch(i, rec, kl_net, trainer=trainer)
                    with self._lock:
                        self.trainer_history.append(rec)
                self._sgf_done.set()
                batches_done = max(n_sgf, int(resumed.get("batches_done", 0)))
                while not stop:
                    items = [self._train_q.get()]
                    while True:
                        try:
                            items.append(self._train_q.get_nowait())
                        except queue.Empty:
                            break
                    for it in items:
                        if it is None:
                            stop = True
                            continue
                        if isinstance(it[0], str):      # the checkpoint marker: the buffer holds exactly the games before the cut
                            self._write_async_checkpoint(it[1], it[2], trainer, games_recv, batches_done)
                            continue
                        self._buffer_block(*it[:3])
                        games_recv += it[3]
                    due = n_sgf + games_recv // self.play_batch_size - batches_done
                    if due <= 0:
                        continue
                    first = batches_done
                    batches_done += due
                    rec = {"batch": batches_done, "buffer": len(self.data_buffer)}
                    if len(self.data_buffer) > self.batch_size:
                        now = time.time()
                        if now < busy_until and not stop:
                            time.sleep(busy_until - now)            # max_update_share: leave the device to self-play
                        if self.exclusive_updates:
                            self._gpu_gate.clear()                  # the self-play loop of this rank waits at its next round
                        try:
                            t0, t1 = self._async_update(trainer, kl_net, rec, skipped=due - 1)
                        finally:
                            self._gpu_gate.set()
                        if self.max_update_share < 1.0:
                            busy_until = t1 + (t1 - t0) * (1.0 / max(self.max_update_share, 1e-3) - 1.0)
                    self._schedule_after_batch(batches_done - 1, rec, kl_net, first=first, trainer=trainer)
                    with self._lock:
                        self.trainer_history.append(rec)
        except BaseException as e:          # surfaces in the main thread at the next round (or in the bootstrap hold)
            self._trainer_error = e
            self._sgf_done.set()

    def _sgf_phase_batches(self):
        """How many leading game batches replay SGF records (0 without records), never more than game_batch_num."""
        return min(int(self.sgf_batches), int(self.game_batch_num)) if self._training_data else 0

    def _async_update(self, trainer, kl_net, rec, skipped=0):
        """One update on the trainer thread: policy_update, the snapshot the next round installs, the counters the round
        header carries (skipped: game batches this update covers beyond its own) and the record -> its (start, end) wall
        clock"""
        t0 = time.time()
        loss, entropy, kl = self.policy_update(trainer, kl_net)
        snap = self._snapshot(trainer)
        t1 = time.time()
        self.update_intervals.append((t0, t1))
        with self._lock:
            self.updates_done += 1
            self.updates_skipped += skipped
            self._last = (loss, entropy, kl)
            self._fresh = (self.updates_done, snap)
        rec.update(loss=loss, entropy=entropy, kl=kl)
        self._note_overflows(rec, trainer)
        return t0, t1

    def _snapshot(self, trainer):
        """A private copy of the trainer's weights for the main thread to broadcast / load while the trainer goes on
        (ema_decay: of its averaged weights)."""
        snap = trainer_weights(trainer, self.ema_decay is not None)
        if hasattr(next(iter(snap.values())), "clone"):         # the trainer's own device tensors
            snap = {k: v.clone() for k, v in snap.items()}
            trainer.torch.cuda.current_stream(trainer.device).synchronize()
        return snap

    def _install_weights(self, version, snap):
        """One round's weight exchange: rank 0 sends snapshot `snap`, everybody (rank 0 included) loads it into the
        self-play evaluator."""
        net = self.policy_value_net
        src = snap if self.rank == 0 else self._param_template()
        got = dist.broadcast_params({k: src[k] for k in sorted(src)}, src=0) if self.distributed else dict(src)
        self._held = load_weights(net, got, keep_trainer=self._custom_net) or self._held
        self._calibrate_after_install()
        self.weights_version = version
        self.weight_broadcasts += 1

    def _run_async(self):
        lead = self.rank == 0
        # the SGF bootstrap batches (rank 0's trainer thread) count as game batches, like the reference's loop index
        target_games = (self.game_batch_num - self._sgf_phase_batches()) * self.play_batch_size * self.world
        if self._async_resume is None:
            self.trainer_history = []
            self._games_collected = 0
            self._round = 0
        if lead:
            self._train_q = queue.Queue()
            self.engine.gate = self._gpu_gate if self.exclusive_updates else None
            self._trainer_thread = threading.Thread(target=self._trainer_main, name="apz-trainer", daemon=True)
            self._trainer_thread.start()
        # The SGF bootstrap first (train_mxnet.py:268-272: self-play starts from the net the game records trained): every
        # rank holds here until rank 0's trainer thread reports the bootstrap batches done.  One short header round trip per
        # interval: no rank sits in a single collective for long, and a trainer failure travels with it.
        bootstrap = self._sgf_phase_batches() > 0
        while True:
            flags = [1.0, 0.0]
            if lead:
                ready = self._sgf_done.wait(timeout=0.5)
                flags = [1.0 if ready else 0.0, 1.0 if self._trainer_error is not None else 0.0]
            if self.distributed:
                flags = dist.broadcast_floats(flags, src=0)
            if flags[1] != 0.0:
                raise RuntimeError("the trainer thread died on rank 0") from (self._trainer_error if lead else None)
            if flags[0] != 0.0:
                break
        rnd = self._round
        stop = False
        draining = False            # the budget is reached and rank 0's trainer works off its queue: rounds without play
        while not stop:
            rnd += 1
            if draining:
                time.sleep(0.2)     # (short header rounds instead of one long wait inside a collective: dist's watchdog)
            elif not (bootstrap and rnd == 1):      # round 1 after a bootstrap only installs the bootstrap's weights
                self._play_round()
            eps = [] if draining else self.engine.finished[:]
            del self.engine.finished[:len(eps)]
            self._taken += len(eps)
            if eps:
                self.episode_len = int(np.mean([len(e.moves) for e in eps]))
            codes, pis, zs = self._episodes_block(eps)
            n_games = len(eps)
            if self.distributed and not draining:
                n_games = int(round(dist.all_reduce_sum(len(eps))))
                codes, pis, zs = dist.all_gather_tuples(codes, pis, zs, consumer=0)      # THE exchange of the round
            self.last_gathered = n_games
            head = [0.0] * 10
            fresh = None
            failed = False
            if lead:
                self._games_collected += n_games
                if len(zs) and self._trainer_error is None:
                    self._train_q.put((codes, pis, zs, n_games))
                cut = 0
                if self.checkpoint_every and n_games and not draining and self._trainer_error is None:
                    unit = self.checkpoint_every * self.play_batch_size
                    if self._games_collected // unit > (self._games_collected - n_games) // unit:
                        cut = self._games_collected // unit
                if cut:
                    # the cut is this round boundary: rank 0's engine now, every other rank's behind the header, the
                    # trainer's side when its thread reaches the marker behind this round's data -- nobody waits for it
                    path = self._async_checkpoint_path(cut)
                    checkpoint.begin(path)
                    self._round = rnd
                    self._write_selfplay_part(checkpoint.tmp_path(path))
                    self._train_q.put(("checkpoint", path, self._main_state()))
                done = self._games_collected >= target_games
                state = 0.0
                if done and self._trainer_error is None:
                    if not draining:
                        self._train_q.put(None)              # drain: the trainer finishes its queue and leaves
                    self._trainer_thread.join(timeout=0.0 if self.distributed else None)
                    state = 2.0 if self._trainer_thread.is_alive() else 1.0
                failed = self._trainer_error is not None        # travels in the header: every rank leaves the loop together
                with self._lock:
                    fresh, self._fresh = self._fresh, None
                    loss, entropy, kl = self._last
                    head = [state, float(fresh[0]) if fresh else float(self.weights_version),
                            float(self.updates_done), loss, entropy, kl, self.lr_multiplier, float(self._games_collected),
                            float(self.updates_skipped), float(cut)]
                if failed:
                    head[0] = -1.0
            if self.distributed:
                head = dist.broadcast_floats(head, src=0)
            if head[0] < 0.0:
                # rank 0 raises with the cause; the others raise too instead of blocking in the next collective
                raise RuntimeError("the trainer thread died on rank 0") from (self._trainer_error if lead else None)
            if head[9] > 0.0 and not lead:
                self._write_selfplay_part(checkpoint.tmp_path(self._async_checkpoint_path(int(head[9]))))
            version = int(head[1])
            rec = {"round": rnd, "games": n_games, "games_collected": int(head[7]), "version": version,
                   "updates": int(head[2]), "updates_skipped": int(head[8]), "leaf_evals": int(self.engine.stats["leaf_evals"])}
            if version > self.weights_version:
                self._install_weights(version, fresh[1] if fresh else None)
                rec.update(loss=head[3], entropy=head[4], kl=head[5], lr_multiplier=head[6])
            self._note_act_scale(rec)
            self.round_log.append((time.time(), int(self.engine.stats["leaf_evals"])))
            self.history.append(rec)
            stop = head[0] == 1.0
            draining = head[0] == 2.0
        return self.history

    def _async_checkpoint_path(self, cut):
        return os.path.join(self.checkpoint_dir, "ckpt_%08d" % (int(cut) * self.checkpoint_every))

    def _write_async_checkpoint(self, path, main_state, trainer, games_recv, batches_done):
        """Rank 0's trainer thread, at the marker: its own parts, then -- once every rank's self-play part is there --
        state.json and COMPLETE"""
        tmp = checkpoint.tmp_path(path)
        self._write_trainer_parts(tmp, trainer)
        state = dict(main_state)
        with self._lock:
            state.update(self._schedule_state())
        state.update(games_recv=int(games_recv), trainer_batches_done=int(batches_done))
        t_end = time.time() + 120.0
        while not all(checkpoint.has_part(tmp, "selfplay_rank%d" % r) for r in range(self.world)):
            if time.time() > t_end:
                _logger.error("checkpoint %s abandoned: a rank's self-play part did not arrive", path)
                return
            time.sleep(0.05)
        checkpoint.finish(path, state)
        checkpoint.prune(self.checkpoint_dir, self.checkpoint_keep)
        _logger.info("checkpoint %s", path)

    def close(self):
        self.engine.close()
        self.policy_value_net.close()
        if self._own_eval_net:
            self._eval_net.close()
        tr = self._async_trainer
        if tr is not None and tr is not self._trainer_override and hasattr(tr, "close"):
            tr.close()


class _KeepTrainer(object):
    """policy_update's evaluator: the net's own HIP inference engine, re-folded from the trainer's weights without
    dropping the trainer's optimiser state."""

    def __init__(self, net):
        self.net = net
        if hasattr(net, "policy_value_dev"):        # planes in device memory (replay "device"): only where the net has it
            self.policy_value_dev = net.policy_value_dev

    def policy_value(self, states):
        return self.net.policy_value(states)

    def set_params(self, prm):
        self.net.set_params(prm, _keep_trainer=True)

    def load_device_params(self, tensors, stream=None):
        self.net.load_device_params(tensors, stream)


class _NoPlayer(object):
    def reset_player(self):
        pass
