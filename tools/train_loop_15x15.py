#!/usr/bin/env python3
"""The reference's training configuration (conf/train_config.yaml: 15x15, 5-in-row, n_playout 400, c_puct 5, batch 128,
8 epochs per update, learn_rate 4e-4, kl_targ 0.02, one policy update per finished self-play game, pure-MCTS opponent
with 1000 playouts) on ONE MI355X, asynchronous schedule (alphapig_amd/pipeline.py): 1024 concurrent self-play games
step on while the trainer thread updates; every published version is installed device to device.
Prints one JSON line per reporting window (profiles/r04_train_loop_15x15.log); --lock-step runs round 3's loop;
--max-update-share caps the share of the wall clock the trainer may be busy; --checkpoint-every / --checkpoint-dir / --resume
write checkpoints and continue from one (the final line lists what every written part cost); --side S runs the same loop
on a framed board (6, 7, 9, 11 .. 14: TrainPipeline train_framed, forced opening off), n_in_row 5."""
import argparse
import json
import os
import resource
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from alphapig_amd.pipeline import TrainPipeline  # noqa: E402


def _time_trainer_thread(tp):
    """Wall clock the trainer thread spends filling the replay buffer (codes_to_planes + get_equi_data + extend, or
    extend_codes), drawing a mini-batch (sample) and inside train_step -> a dict that fills while the loop runs.  What is
    left of the update intervals beside sample and train_step is the KL monitor and the weight snapshot."""
    import threading
    from alphapig_amd import pipeline, train
    acc = {"fill_s": 0.0, "sample_s": 0.0, "train_step_s": 0.0}

    def timed(fn, key):
        def inner(*a, **kw):
            if threading.current_thread().name != "apz-trainer":
                return fn(*a, **kw)
            t = time.perf_counter()
            try:
                return fn(*a, **kw)
            finally:
                acc[key] += time.perf_counter() - t
        return inner
    buf = tp.data_buffer
    buf.sample = timed(buf.sample, "sample_s")
    if tp.replay == "tuples":
        buf.extend = timed(buf.extend, "fill_s")
        pipeline.get_equi_data = timed(pipeline.get_equi_data, "fill_s")
        tp.engine.pool.codes_to_planes = timed(tp.engine.pool.codes_to_planes, "fill_s")
    else:
        buf.extend_codes = timed(buf.extend_codes, "fill_s")
    train.HipTrainer.train_step = timed(train.HipTrainer.train_step, "train_step_s")
    return acc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=1500, help="game batches (= games: play_batch_size 1) to collect")
    ap.add_argument("--report-s", type=float, default=20.0)
    ap.add_argument("--max-update-share", type=float, default=1.0)
    ap.add_argument("--lock-step", action="store_true")
    ap.add_argument("--exclusive", action="store_true", help="no new self-play round while the trainer is inside a policy update (default: interleaved)")
    ap.add_argument("--eval-games", type=int, default=10)
    ap.add_argument("--pure-playouts", type=int, default=1000)
    ap.add_argument("--train-arith", default="f32", choices=("f32", "f16x2"), help="the trainer's trunk arithmetic (HipTrainer trunk_arith)")
    ap.add_argument("--act-scale", default="off", choices=("off", "auto"),
                    help="the self-play evaluator's static activation exponents (TrainPipeline act_scale)")
    ap.add_argument("--replay", default="tuples", choices=("tuples", "compact", "device"),
                    help="what the replay buffer stores (TrainPipeline replay): augmented tuples, codes on the host, codes on the GPU")
    ap.add_argument("--checkpoint-every", type=int, default=0, help="game batches between two checkpoints (0: none)")
    ap.add_argument("--checkpoint-dir", default=None, help="where they go (default: <model_dir>/checkpoints)")
    ap.add_argument("--checkpoint-selfplay", default="games", choices=("games", "none"),
                    help="save the games in flight with their trees, or abandon them")
    ap.add_argument("--side", type=int, default=15, help="board side: 15, or a framed side (6, 7, 9, 11 .. 14) with train_framed")
    ap.add_argument("--step-guard", action="store_true",
                    help="skip optimiser steps whose gradients or losses are not finite (TrainPipeline step_guard)")
    ap.add_argument("--clip-norm", type=float, default=None, help="clip the global gradient norm (TrainPipeline clip_norm; implies --step-guard)")
    ap.add_argument("--legal-policy", action="store_true",
                    help="policy softmax and loss over the empty cells of every position (TrainPipeline legal_policy)")
    ap.add_argument("--resume", default=None, help="a checkpoint directory, or 'latest' for the newest complete one in --checkpoint-dir")
    args = ap.parse_args()
    conf = dict(board_width=args.side, board_height=args.side, train_framed=args.side != 15, n_in_row=5, learn_rate=4e-4, lr_multiplier=1.0, temp=1.0,
                n_playout=400, c_puct=5, buffer_size=2198800, batch_size=128, epochs=8, kl_targ=0.02,
                check_freq=10 ** 9, pure_mcts_playout_num=args.pure_playouts, game_batch_num=args.games,
                play_batch_size=1, concurrent_games=1024, n_blocks=10, n_filter=128, eval_games=args.eval_games,
                model_dir="/tmp/apz_models_15", async_update=not args.lock_step, round_seconds=0.25,
                max_update_share=args.max_update_share, exclusive_updates=args.exclusive, train_arith=args.train_arith,
                act_scale=args.act_scale, replay=args.replay, checkpoint_every=args.checkpoint_every,
                checkpoint_dir=args.checkpoint_dir, checkpoint_selfplay=args.checkpoint_selfplay,
                step_guard=args.step_guard, clip_norm=args.clip_norm, legal_policy=args.legal_policy)
    resume = args.resume
    if resume == "latest":
        from alphapig_amd import checkpoint
        done = checkpoint.complete_checkpoints(args.checkpoint_dir or os.path.join(conf["model_dir"], "checkpoints"))
        resume = done[-1] if done else None
    tp = TrainPipeline(conf, seed=1, resume=resume)
    host = _time_trainer_thread(tp)
    t0 = time.time()
    if args.lock_step:
        hist = tp.run()
        print(json.dumps({"mode": "lock step", "batches": len(hist), "seconds": round(time.time() - t0, 1),
                          "leaf_evals_per_s": round(tp.engine.stats["leaf_evals"] / (time.time() - t0))}), flush=True)
        tp.close()
        return
    # report from a side thread: the pipeline's own loop is not interrupted
    import threading
    stop = threading.Event()

    def reporter():
        last_t, last_leaf, last_busy, last_upd, last_games = t0, 0, 0.0, 0, 0
        while not stop.wait(args.report_s):
            now = time.time()
            leaf = tp.engine.stats["leaf_evals"]
            iv = list(tp.update_intervals)
            busy = sum(b - a for a, b in iv)
            games = tp._taken
            rec = {"seconds": round(now - t0, 1), "games_taken": games,
                   "games_per_s_this_window": round((games - last_games) / (now - last_t), 2),
                   "leaf_evals_per_s_this_window": round((leaf - last_leaf) / (now - last_t)),
                   "updates_done": tp.updates_done, "updates_skipped": tp.updates_skipped,
                   "policy_update_ms": round(1e3 * (busy - last_busy) / max(1, len(iv) - last_upd), 1),
                   "update_share_of_wall": round((busy - last_busy) / (now - last_t), 3), "buffer": len(tp.data_buffer),
                   "weights_version": tp.weights_version, "lr_multiplier": round(tp.lr_multiplier, 3)}
            ups = [h for h in getattr(tp, "trainer_history", []) if "loss" in h]
            if ups:
                rec.update(loss=round(ups[-1]["loss"], 4), entropy=round(ups[-1]["entropy"], 4), kl=round(ups[-1]["kl"], 5))
                if "trunk_overflows" in ups[-1]:
                    rec["trunk_overflows"] = ups[-1]["trunk_overflows"]
            if tp.history:                      # the self-play evaluator's repeats (and exponents with --act-scale auto)
                for k in ("eval_trunk_overflows", "act_exponents"):
                    if k in tp.history[-1]:
                        rec[k] = tp.history[-1][k]
            print(json.dumps(rec), flush=True)
            last_t, last_leaf, last_busy, last_upd, last_games = now, leaf, busy, len(iv), games

    th = threading.Thread(target=reporter, daemon=True)
    th.start()
    tp.run()
    stop.set()
    dt = time.time() - t0
    print(json.dumps({"mode": "asynchronous", "max_update_share": args.max_update_share, "seconds": round(dt, 1),
                      "games": tp._taken, "updates_done": tp.updates_done, "updates_skipped": tp.updates_skipped,
                      "leaf_evals_per_s_whole_run": round(tp.engine.stats["leaf_evals"] / dt),
                      "update_share_of_wall_whole_run": round(sum(b - a for a, b in tp.update_intervals) / dt, 3),
                      "exclusive_updates": tp.exclusive_updates, "replay": tp.replay,
                      "trainer_thread_s": {k: round(v, 3) for k, v in host.items()},
                      "peak_rss_mb": round(resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 1024.0, 1),
                      "self_play_held_s": round(tp.engine.timers.get("gate_s", 0.0), 2), "train_arith": tp.train_arith,
                      "policy_update_ms_whole_run": round(1e3 * sum(b - a for a, b in tp.update_intervals) /
                                                          max(1, len(tp.update_intervals)), 1),
                      "trunk_overflows": getattr(getattr(tp, "_async_trainer", None), "trunk_overflows", None),
                      "checkpoint_parts": [{"part": p, "seconds": round(t, 3), "bytes": b} for p, t, b in tp.checkpoint_log],
                      "tree_peak_nodes": tp.engine.pool.pool_info()["peak_nodes"],
                      "act_scale": tp.act_scale, "eval_trunk_overflows": tp.policy_value_net.trunk_overflows(),
                      "act_exponents": tp.policy_value_net.trunk_act_exponents() if tp.act_scale == "auto" else None}),
          flush=True)
    tp.close()


if __name__ == "__main__":
    main()
