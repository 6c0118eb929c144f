#!/usr/bin/env python3
"""Training-step timing on the GPU box: the product trainer (alphapig_amd/train.py, every operator a HIP kernel of
this repository) beside the same graph in PyTorch (MIOpen convolutions; tests/torch_trainer.py, the comparator the
trainer is tested against), 10-block net, 15x15.  --arith f32,f16x2: the product trainer with each trunk arithmetic
(HipTrainer trunk_arith), the two alternating --reps times on the same box, step times side by side.  --side 15,9,13: the
product trainer per board side (framed sides: HipTrainer framed=True), alternating in one process in the same way, each
side's step time and its ratio to the first.  --step-guard: the product trainer without and with the guarded optimiser step
(HipTrainer step_guard; --clip-norm adds clipping), alternating in the same way, per --arith arithmetic (default f32).
--ema: the product trainer without and with the averaged weights (HipTrainer ema_decay; --ema-decay), alternating in the same
way, and the averaging launch on its own between two events.  --legal-policy: the product trainer without and with the
legal-move policy (HipTrainer legal_policy: the occupancy launch per uploaded batch, the masked loss), alternating in the same way."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from alphapig_amd import weights  # noqa: E402
from alphapig_amd.train import HipTrainer  # noqa: E402


def main():
    import torch
    from torch_trainer import TorchTrainer
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="128,512")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--arith", default=None, help="comma list of HipTrainer trunk arithmetics (f32,f16x2): alternating runs")
    ap.add_argument("--reps", type=int, default=3, help="--arith / --side: alternating repetitions")
    ap.add_argument("--side", default=None, help="comma list of board sides (15 and framed sides 6, 7, 9, 11 .. 14): alternating runs")
    ap.add_argument("--step-guard", action="store_true", help="HipTrainer step_guard off / on: alternating runs")
    ap.add_argument("--clip-norm", type=float, default=None, help="--step-guard: the guarded trainer's clip_norm")
    ap.add_argument("--ema", action="store_true", help="HipTrainer ema_decay off / on: alternating runs")
    ap.add_argument("--ema-decay", type=float, default=0.999, help="--ema: the averaging trainer's ema_decay")
    ap.add_argument("--legal-policy", action="store_true", help="HipTrainer legal_policy off / on: alternating runs")
    args = ap.parse_args()
    rs = np.random.RandomState(0)
    prm = weights.init_params("resnet", 15, 15, 9, 10, 128, seed=0, style="bench")
    out = {}
    if args.side:
        return side_ab(args, rs)
    if args.ema:
        return ema_ab(args, prm, rs)
    if args.legal_policy:
        return legal_ab(args, prm, rs)
    if args.step_guard:
        return guard_ab(args, prm, rs)
    if args.arith:
        return arith_ab(args, prm, rs)
    for B in [int(x) for x in args.batches.split(",")]:
        states = (rs.rand(B, 9, 15, 15) > 0.7).astype(np.float32)
        pis = rs.dirichlet(np.ones(225), size=B).astype(np.float32)
        zs = rs.choice([-1.0, 1.0], size=B).astype(np.float32)
        for backend in ("hip",) if args.no_torch else ("torch", "hip"):
            if backend == "hip":
                tr = HipTrainer(prm, "resnet", n_blocks=10, batch_size=B)
            else:
                tr = TorchTrainer(prm, "resnet", n_blocks=10, batch_size=B, device="cuda")
            for _ in range(3):
                tr.train_step(states, pis, zs, 1e-3)
            torch.cuda.synchronize()
            t = time.perf_counter()
            for _ in range(args.steps):
                tr.train_step(states, pis, zs, 1e-3)
            torch.cuda.synchronize()
            ms = 1e3 * (time.perf_counter() - t) / args.steps
            flops = 3 * 2.0 * B * (9 * 128 + 20 * 128 * 128) * 9 * 225       # fwd + dgrad + wgrad of the 3x3 convs
            out["B%d_%s" % (B, backend)] = {"ms_per_step": ms, "conv_tflops_equiv": flops / ms / 1e9}
            print("batch %4d  %-6s  %.2f ms/step   (3x3-conv work %.1f TFLOP/s equivalent)" %
                  (B, backend, ms, flops / ms / 1e9), flush=True)
            if backend == "hip":     # what epochs 2 .. n of a policy_update pay: the mini-batch is on the device already
                batch = tr.upload(states, pis, zs)
                tr.train_step(batch, None, None, 1e-3)
                torch.cuda.synchronize()
                t = time.perf_counter()
                for _ in range(args.steps):
                    tr.train_step(batch, None, None, 1e-3)
                torch.cuda.synchronize()
                ms = 1e3 * (time.perf_counter() - t) / args.steps
                out["B%d_hip_resident_batch" % B] = {"ms_per_step": ms}
                print("batch %4d  hip     %.2f ms/step on an uploaded mini-batch (HipTrainer.upload: policy_update's epochs share one)" %
                      (B, ms), flush=True)
    print(json.dumps(out))


def arith_ab(args, prm, rs):
    """Both trunk arithmetics per batch size, alternating: one trainer each, `--reps` rounds of (warm-up step, `--steps`
    timed steps on an uploaded mini-batch) per arithmetic in turn; the median step time per arithmetic and their ratio."""
    import torch
    ariths = args.arith.split(",")
    out = {}
    for B in [int(x) for x in args.batches.split(",")]:
        states = (rs.rand(B, 9, 15, 15) > 0.7).astype(np.float32)
        pis = rs.dirichlet(np.ones(225), size=B).astype(np.float32)
        zs = rs.choice([-1.0, 1.0], size=B).astype(np.float32)
        trs = {a: HipTrainer(prm, "resnet", n_blocks=10, batch_size=B, trunk_arith=a) for a in ariths}
        batches = {a: trs[a].upload(states, pis, zs) for a in ariths}
        times = {a: [] for a in ariths}
        for _ in range(args.reps):
            for a in ariths:
                tr = trs[a]
                tr.train_step(batches[a], None, None, 1e-3)
                torch.cuda.synchronize()
                t = time.perf_counter()
                for _ in range(args.steps):
                    tr.train_step(batches[a], None, None, 1e-3)
                torch.cuda.synchronize()
                times[a].append(1e3 * (time.perf_counter() - t) / args.steps)
        med = {a: float(np.median(times[a])) for a in ariths}
        for a in ariths:
            out["B%d_%s" % (B, a)] = {"ms_per_step": med[a], "runs_ms": [round(x, 3) for x in times[a]],
                                      "trunk_overflows": getattr(trs[a], "trunk_overflows", 0)}
        print("batch %4d  " % B + "   ".join("%s %.3f ms/step (runs %s)" % (a, med[a], ", ".join("%.3f" % x for x in times[a]))
                                           for a in ariths) +
              ("   ratio %s/%s %.3f" % (ariths[1], ariths[0], med[ariths[1]] / med[ariths[0]]) if len(ariths) > 1 else ""),
              flush=True)
        for tr in trs.values():
            tr.close()
    print(json.dumps(out))


def guard_ab(args, prm, rs):
    """The step without and with the guard per batch size (and --arith arithmetic), alternating like arith_ab: one trainer
    each from the same weights, `--reps` rounds of (warm-up step, `--steps` timed steps on an uploaded mini-batch) in turn;
    the median step time of each, all runs (their spread is the yardstick for the difference), the guarded trainer's
    counters."""
    import torch
    out = {}
    for B in [int(x) for x in args.batches.split(",")]:
        states = (rs.rand(B, 9, 15, 15) > 0.7).astype(np.float32)
        pis = rs.dirichlet(np.ones(225), size=B).astype(np.float32)
        zs = rs.choice([-1.0, 1.0], size=B).astype(np.float32)
        for a in (args.arith or "f32").split(","):
            trs = {"plain": HipTrainer(prm, "resnet", n_blocks=10, batch_size=B, trunk_arith=a),
                   "guarded": HipTrainer(prm, "resnet", n_blocks=10, batch_size=B, trunk_arith=a, step_guard=True,
                                         clip_norm=args.clip_norm)}
            batches = {k: tr.upload(states, pis, zs) for k, tr in trs.items()}
            times = {k: [] for k in trs}
            for _ in range(args.reps):
                for k, tr in trs.items():
                    tr.train_step(batches[k], None, None, 1e-3)
                    torch.cuda.synchronize()
                    t = time.perf_counter()
                    for _ in range(args.steps):
                        tr.train_step(batches[k], None, None, 1e-3)
                    torch.cuda.synchronize()
                    times[k].append(1e3 * (time.perf_counter() - t) / args.steps)
            med = {k: float(np.median(times[k])) for k in trs}
            g = trs["guarded"]
            for k in trs:
                out["B%d_%s_%s" % (B, a, k)] = {"ms_per_step": med[k], "runs_ms": [round(x, 3) for x in times[k]]}
            out["B%d_%s_guarded" % (B, a)].update(skipped_steps=g.skipped_steps, clipped_steps=g.clipped_steps,
                                                  grad_norm=g.last_grad_norm)
            print("batch %4d %-5s  " % (B, a) +
                  "   ".join("%s %.3f ms/step (runs %s)" % (k, med[k], ", ".join("%.3f" % x for x in times[k])) for k in trs) +
                  "   ratio guarded/plain %.4f   grad_norm %.4g skipped %d clipped %d" %
                  (med["guarded"] / med["plain"], g.last_grad_norm, g.skipped_steps, g.clipped_steps), flush=True)
            for tr in trs.values():
                tr.close()
    print(json.dumps(out))


def legal_ab(args, prm, rs):
    """The step without and with the legal-move policy per batch size (and --arith arithmetic), alternating like guard_ab: one
    trainer each from the same weights, `--reps` rounds of (warm-up step, `--steps` timed steps on an uploaded mini-batch) in
    turn; the median step time of each and all runs (their spread is the yardstick for the difference).  The planes are random
    bits at density 0.3, so half the cells carry a stone; pi is zero there."""
    import torch
    out = {}
    for B in [int(x) for x in args.batches.split(",")]:
        states = (rs.rand(B, 9, 15, 15) > 0.7).astype(np.float32)
        occ = ((states[:, 6] != 0) | (states[:, 7] != 0))[:, ::-1].reshape(B, 225)
        pis = rs.dirichlet(np.ones(225), size=B) * ~occ
        pis = (pis / pis.sum(axis=1, keepdims=True)).astype(np.float32)
        zs = rs.choice([-1.0, 1.0], size=B).astype(np.float32)
        for a in (args.arith or "f32").split(","):
            trs = {"plain": HipTrainer(prm, "resnet", n_blocks=10, batch_size=B, trunk_arith=a),
                   "legal": HipTrainer(prm, "resnet", n_blocks=10, batch_size=B, trunk_arith=a, legal_policy=True)}
            batches = {k: tr.upload(states, pis, zs) for k, tr in trs.items()}
            times = {k: [] for k in trs}
            for _ in range(args.reps):
                for k, tr in trs.items():
                    tr.train_step(batches[k], None, None, 1e-3)
                    torch.cuda.synchronize()
                    t = time.perf_counter()
                    for _ in range(args.steps):
                        tr.train_step(batches[k], None, None, 1e-3)
                    torch.cuda.synchronize()
                    times[k].append(1e3 * (time.perf_counter() - t) / args.steps)
            med = {k: float(np.median(times[k])) for k in trs}
            for k in trs:
                out["B%d_%s_%s" % (B, a, k)] = {"ms_per_step": med[k], "runs_ms": [round(x, 3) for x in times[k]]}
            print("batch %4d %-5s  " % (B, a) +
                  "   ".join("%s %.3f ms/step (runs %s)" % (k, med[k], ", ".join("%.3f" % x for x in times[k])) for k in trs) +
                  "   ratio legal/plain %.4f" % (med["legal"] / med["plain"]), flush=True)
            for tr in trs.values():
                tr.close()
    print(json.dumps(out))


def ema_ab(args, prm, rs):
    """The step without and with the averaged weights per batch size (and --arith arithmetic), alternating like guard_ab: one
    trainer each from the same weights, `--reps` rounds of (warm-up step, `--steps` timed steps on an uploaded mini-batch) in
    turn; the median step time of each and all runs (their spread is the yardstick for the difference).  Then the averaging
    launch alone: 100 launches between two events, `--reps` times -- back to back, so the 25 MB it reads and the 12.7 MB it
    writes may still sit in the last-level cache from the launch before; behind a training step they come from HBM."""
    import torch
    out = {}
    for B in [int(x) for x in args.batches.split(",")]:
        states = (rs.rand(B, 9, 15, 15) > 0.7).astype(np.float32)
        pis = rs.dirichlet(np.ones(225), size=B).astype(np.float32)
        zs = rs.choice([-1.0, 1.0], size=B).astype(np.float32)
        for a in (args.arith or "f32").split(","):
            trs = {"plain": HipTrainer(prm, "resnet", n_blocks=10, batch_size=B, trunk_arith=a),
                   "ema": HipTrainer(prm, "resnet", n_blocks=10, batch_size=B, trunk_arith=a, ema_decay=args.ema_decay)}
            batches = {k: tr.upload(states, pis, zs) for k, tr in trs.items()}
            times = {k: [] for k in trs}
            for _ in range(args.reps):
                for k, tr in trs.items():
                    tr.train_step(batches[k], None, None, 1e-3)
                    torch.cuda.synchronize()
                    t = time.perf_counter()
                    for _ in range(args.steps):
                        tr.train_step(batches[k], None, None, 1e-3)
                    torch.cuda.synchronize()
                    times[k].append(1e3 * (time.perf_counter() - t) / args.steps)
            med = {k: float(np.median(times[k])) for k in trs}
            e = trs["ema"]
            launch_us = []
            for _ in range(args.reps):
                e._ema()
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for _ in range(100):
                    e._ema()
                t1.record()
                torch.cuda.synchronize()
                launch_us.append(1e3 * t0.elapsed_time(t1) / 100)
            for k in trs:
                out["B%d_%s_%s" % (B, a, k)] = {"ms_per_step": med[k], "runs_ms": [round(x, 3) for x in times[k]]}
            nbytes = 12 * sum(v.numel() for v in e.p.values())
            out["B%d_%s_ema" % (B, a)].update(ema_updates=e.ema_updates, launch_us=[round(x, 2) for x in launch_us],
                                              launch_bytes=nbytes)
            print("batch %4d %-5s  " % (B, a) +
                  "   ".join("%s %.3f ms/step (runs %s)" % (k, med[k], ", ".join("%.3f" % x for x in times[k])) for k in trs) +
                  "   ratio ema/plain %.4f   launch alone %s us (%.1f MB moved)   ema_updates %d" %
                  (med["ema"] / med["plain"], ", ".join("%.2f" % x for x in launch_us), nbytes / 1e6, e.ema_updates), flush=True)
            for tr in trs.values():
                tr.close()
    print(json.dumps(out))


def side_ab(args, rs):
    """The step per board side and batch size, alternating like arith_ab: one trainer per side, `--reps` rounds of (warm-up
    step, `--steps` timed steps on an uploaded mini-batch) per side in turn; the median step time per side and its ratio to
    the first side's."""
    import torch
    sides = [int(x) for x in args.side.split(",")]
    out = {}
    for B in [int(x) for x in args.batches.split(",")]:
        trs, batches, times = {}, {}, {S: [] for S in sides}
        for S in sides:
            prm = weights.init_params("resnet", S, S, 9, 10, 128, seed=0, style="bench")
            trs[S] = HipTrainer(prm, "resnet", n_blocks=10, batch_size=B, framed=True)
            batches[S] = trs[S].upload((rs.rand(B, 9, S, S) > 0.7).astype(np.float32),
                                       rs.dirichlet(np.ones(S * S), size=B).astype(np.float32),
                                       rs.choice([-1.0, 1.0], size=B).astype(np.float32))
        for _ in range(args.reps):
            for S in sides:
                trs[S].train_step(batches[S], None, None, 1e-3)
                torch.cuda.synchronize()
                t = time.perf_counter()
                for _ in range(args.steps):
                    trs[S].train_step(batches[S], None, None, 1e-3)
                torch.cuda.synchronize()
                times[S].append(1e3 * (time.perf_counter() - t) / args.steps)
        med = {S: float(np.median(times[S])) for S in sides}
        for S in sides:
            out["B%d_side%d" % (B, S)] = {"ms_per_step": med[S], "runs_ms": [round(x, 3) for x in times[S]],
                                          "ratio_to_side%d" % sides[0]: round(med[S] / med[sides[0]], 4)}
        print("batch %4d  " % B + "   ".join("%dx%d %.3f ms/step (x%.3f; runs %s)" % (S, S, med[S], med[S] / med[sides[0]],
                                                                                     ", ".join("%.3f" % x for x in times[S]))
                                           for S in sides), flush=True)
        for tr in trs.values():
            tr.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
