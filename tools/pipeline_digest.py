#!/usr/bin/env python3
"""sha256 digests of what TrainPipeline's lock-step schedule computes, for comparing two source trees bit by bit:

    python tools/pipeline_digest.py --standin > digest.txt        (CPU; once per tree; diff the two files)
    python tools/pipeline_digest.py > digest.txt                  (GPU)
    python tools/pipeline_digest.py --tree OTHER_TREE ...         (the same file against another checkout)

Only the public surface is used -- TrainPipeline(conf, ...), run(), history, trainer_history, policy_value_net.params(),
checkpoint_every / resume= -- so one copy of this file runs against both trees.  Per case one digest over the JSON of the
history records (trainer_history behind them) and the evaluator's parameters in name order; where a checkpoint is written,
one more over its state.json (minus WALL_CLOCK) and its trainer part.  Lock-step cases only: the asynchronous schedule is
timing-dependent by design.

--standin: tests/_pipeline_worker.py's TiltNet / TiltTrainer on 8x8, 4 in a row, 4 game batches of 2 games, 4 concurrent
games: plain, replay=compact, ema_decay=0.5 with a trainer that keeps an average as NumPy arrays, checkpoint_every=2
followed by a resume to 6 batches, sgf_batches=1 on the golden records.
Without it: PolicyValueNet + HipTrainer, the 8x8 simple net (an evaluator passed in) and a 15x15 resnet of 1 block x 128
(the evaluator the pipeline builds), batch_size 16, n_playout 8, 4 concurrent games, 3 game batches: plain, replay=device,
train_arith=f16x2, step_guard + clip_norm, ema_decay, legal_policy (both nets: the fused 8x8 head, the two-launch head and
the loss in their legal-move forms), act_scale=auto, train_framed on side 6, checkpoint and resume.  The same run under rocprofv3 --kernel-trace is the launch sequence tools/route_trace.py --compare --whole compares.

--workdir DIR keeps the checkpoints under DIR/<case>/; --checkpoints-from DIR2 makes every resume read the checkpoint
another run (another tree's) left under DIR2/<case>/ instead of its own: both must continue to the same digest."""
import argparse
import hashlib
import json
import os
import sys
import tempfile

import numpy as np

WALL_CLOCK = ("update_intervals", "round_log", "checkpoint_log")


def digest(history, params):
    h = hashlib.sha256()
    h.update(json.dumps(history, sort_keys=True).encode())
    for k in sorted(params):
        a = np.ascontiguousarray(params[k])
        h.update(("%s %s %s;" % (k, a.dtype, a.shape)).encode())
        h.update(a.tobytes())
    return h.hexdigest()


def checkpoint_digest(checkpoint, path):
    state = {k: v for k, v in checkpoint.read_state(path).items() if k not in WALL_CLOCK}
    part = checkpoint.read_part(path, "trainer")
    state["trainer meta"] = part.pop("meta")
    return digest(state, part)


def report(label, pipe):
    hist = list(pipe.history) + list(pipe.trainer_history)
    print("%-44s %s  %d records, %d updates" % (label, digest(hist, pipe.policy_value_net.params()), len(pipe.history),
                                                 sum("loss" in r for r in hist)), flush=True)


def base_conf(work, **kw):
    c = {"board_width": 8, "board_height": 8, "n_in_row": 4, "learn_rate": 2e-3, "lr_multiplier": 1.0, "temp": 1.0,
         "n_playout": 8, "c_puct": 5, "buffer_size": 1000, "batch_size": 16, "epochs": 2, "kl_targ": 0.02,
         "check_freq": 1000, "game_batch_num": 4, "play_batch_size": 2, "pure_mcts_playout_num": 10, "async_update": False,
         "concurrent_games": 4, "model_dir": os.path.join(work, "models")}
    c.update(kw)
    return c


def run_case(label, make, conf, args, resume_to=None):
    """make(conf, resume) -> a pipeline.  resume_to: the checkpoint case -- run to game_batch_num with checkpoint_every,
    digest the last checkpoint, then a fresh pipeline resumes from it (or from the other run's) to `resume_to` batches"""
    from alphapig_amd import checkpoint
    try:
        pipe = make(conf, None)
        pipe.run()
        report(label, pipe)
        pipe.close()
        if resume_to is None:
            return
        name = "ckpt_%08d" % conf["game_batch_num"]
        path = os.path.join(conf["model_dir"], "checkpoints", name)
        print("%-44s %s" % (label + ": checkpoint", checkpoint_digest(checkpoint, path)), flush=True)
        if args.checkpoints_from:
            path = os.path.join(args.checkpoints_from, os.path.relpath(path, args.workdir))
        pipe = make(dict(conf, game_batch_num=resume_to, checkpoint_every=0), path)
        pipe.run()
        report(label + ": resumed to %d" % resume_to, pipe)
        pipe.close()
    except ValueError as e:                 # a configuration a tree refuses: the refusal is its line (anything else ends the run)
        print("%-44s %s: %s" % (label, type(e).__name__, e), flush=True)


def standin(args):
    sys.path.insert(0, os.path.join(args.tree, "tests"))
    from _pipeline_worker import TiltNet, TiltTrainer
    from alphapig_amd.pipeline import TrainPipeline

    class StateTilt(TiltTrainer):
        """... that can be checkpointed"""

        def state(self):
            return {"meta": {"t": self.t}, "p/w": self._p["w"].copy(), "p/b": self._p["b"].copy()}

        def load_state(self, state):
            self._p = {k: np.array(state["p/" + k], np.float32) for k in ("w", "b")}
            self.t = int(state["meta"]["t"])

    class EmaTilt(StateTilt):
        """... with HipTrainer's averaged weights as NumPy arrays (decay 0.5, no warm-up) and an evaluator of its own for
        the KL monitor; no torch, no sync_evaluator"""

        def __init__(self, net):
            StateTilt.__init__(self, net)
            self.ema_p = {k: v.copy() for k, v in self._p.items()}
            self.ema_updates = 0
            self.own = TiltNet(len(self._p["w"]))

        def train_step(self, states, pis, zs, lr):
            out = StateTilt.train_step(self, states, pis, zs, lr)
            for k in self.ema_p:
                self.ema_p[k] = (self.ema_p[k] + np.float32(0.5) * (self._p[k] - self.ema_p[k])).astype(np.float32)
            self.ema_updates += 1
            return out

        def ema_params(self):
            return {k: v.copy() for k, v in self.ema_p.items()}

        def policy_value(self, states):
            self.own.set_params(self._p)
            return self.own.policy_value(states)

        def state(self):
            out = StateTilt.state(self)
            out["meta"]["ema_updates"] = self.ema_updates
            out.update({"e/" + k: v.copy() for k, v in self.ema_p.items()})
            return out

        def load_state(self, state):
            StateTilt.load_state(self, state)
            self.ema_p = {k: np.array(state["e/" + k], np.float32) for k in ("w", "b")}
            self.ema_updates = int(state["meta"]["ema_updates"])

    def maker(trainer_cls, hw=64):
        def make(conf, resume):
            net = TiltNet(hw)
            pipe = TrainPipeline(conf, policy_value_net=net, seed=1, trainer=trainer_cls(net), distributed=False, resume=resume)
            pipe.close = pipe.engine.close          # (the stand-in evaluators hold nothing)
            return pipe
        return make

    def conf(case, **kw):
        return base_conf(os.path.join(args.workdir, case), **kw)

    run_case("standin plain", maker(StateTilt), conf("plain"), args)
    run_case("standin replay=compact", maker(StateTilt), conf("compact", replay="compact"), args)
    run_case("standin ema_decay=0.5", maker(EmaTilt), conf("ema", ema_decay=0.5), args)
    run_case("standin checkpoint_every=2", maker(StateTilt), conf("ckpt", checkpoint_every=2, checkpoint_buffer=True), args,
             resume_to=6)
    run_case("standin ema_decay=0.5 checkpoint_every=2", maker(EmaTilt),
             conf("ema_ckpt", ema_decay=0.5, checkpoint_every=2, replay="compact"), args, resume_to=6)
    g = np.load(os.path.join(args.tree, "tests", "golden", "sgf.npz"))
    home = os.path.join(args.workdir, "sgf_records")
    os.makedirs(home, exist_ok=True)
    for k in range(int(g["n"])):
        if not int(g["f%d_warning" % k]):
            with open(os.path.join(home, str(g["f%d_name" % k])), "w", newline="") as f:
                f.write(str(g["f%d_text" % k]))
    import random
    random.seed(5)          # (the pipeline shuffles the record list with the module's generator)
    run_case("standin sgf_batches=1 (15x15)", maker(StateTilt, 225),
             conf("sgf", board_width=15, board_height=15, n_in_row=5, sgf_batches=1, sgf_dir=home, game_batch_num=3,
                  play_batch_size=1, buffer_size=100000), args)


def real(args):
    from alphapig_amd.pipeline import TrainPipeline
    from alphapig_amd.policy_value_net import PolicyValueNet

    def resnet(conf, resume):
        return TrainPipeline(conf, seed=1, distributed=False, resume=resume)

    def simple(conf, resume):
        net = PolicyValueNet(8, 8, batch_size=16, n_blocks=0, net_kind="simple", seed=3)
        return TrainPipeline(conf, policy_value_net=net, seed=1, distributed=False, resume=resume)

    def conf(case, side=15, **kw):
        big = dict(board_width=side, board_height=side, n_in_row=5 if side == 15 else 4, n_blocks=1, n_filter=128)
        return base_conf(os.path.join(args.workdir, case), **{**(big if side != 8 else {}), "game_batch_num": 3, **kw})

    for name, make, side in (("simple 8x8", simple, 8), ("resnet 15x15", resnet, 15)):
        tag = name.split()[0]
        run_case(name + " plain", make, conf(tag + "_plain", side), args)
        run_case(name + " replay=device", make, conf(tag + "_device", side, replay="device"), args)
        run_case(name + " step_guard clip_norm", make, conf(tag + "_guard", side, step_guard=True, clip_norm=0.5), args)
        run_case(name + " ema_decay", make, conf(tag + "_ema", side, ema_decay=0.9), args)
        run_case(name + " checkpoint", make, conf(tag + "_ckpt", side, game_batch_num=2, checkpoint_every=2, replay="compact"),
                 args, resume_to=4)
        run_case(name + " ema_decay checkpoint", make,
                 conf(tag + "_ema_ckpt", side, game_batch_num=2, checkpoint_every=2, ema_decay=0.9, checkpoint_buffer=True), args,
                 resume_to=4)
    run_case("resnet 15x15 train_arith=f16x2", resnet, conf("resnet_f16x2", train_arith="f16x2"), args)
    run_case("simple 8x8 legal_policy", simple, conf("simple_legal", 8, legal_policy=True), args)
    run_case("resnet 15x15 legal_policy", resnet, conf("resnet_legal", legal_policy=True), args)
    run_case("resnet 15x15 act_scale=auto", resnet, conf("resnet_act", act_scale="auto"), args)
    run_case("resnet 6x6 train_framed", resnet, conf("resnet_framed", 6, train_framed=True), args)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--standin", action="store_true", help="the CPU cases on stand-in evaluator and trainer")
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    help="the checkout whose alphapig_amd (and tests/) to run (default: this file's)")
    ap.add_argument("--workdir", default=None, help="where model_dir and the checkpoints of every case go (default: temporary)")
    ap.add_argument("--checkpoints-from", default=None, help="the --workdir of another run: resume from ITS checkpoints")
    args = ap.parse_args()
    args.tree = os.path.abspath(args.tree)
    sys.path.insert(0, args.tree)
    with tempfile.TemporaryDirectory() as tmp:
        args.workdir = os.path.abspath(args.workdir or tmp)
        (standin if args.standin else real)(args)


if __name__ == "__main__":
    main()
