#!/usr/bin/env python3
"""The training step of the generic 15x15 nets, HipTrainer(trunk_arith="f32") against trunk_arith="f16x2" (the 3x3 layers'
forward and data gradient on conv15h_kernel, csrc/conv15_split.h), in ONE process, the two arithmetics ALTERNATING round
after round so that clock and temperature drift falls on both alike.

    python tools/generic_train_bench.py [--batches 128,512] [--rounds 5] [--iters 10] [--warmup 3] [--nets simple15,...]

Steps: train_step on a DeviceBatch uploaded once (what policy_update does), wall clock over `iters` steps after `warmup`
untimed ones; every step ends in its one read-back, so the clock sees whole steps.  Nets: simple15, resnet15x64 and
resnet15x256 with 1 and with 10 blocks.  Reported: the mean over the rounds and the spread of the per-round means, and
f16x2 / f32 (below 1: the f16x2 step is faster).
Data gradient: one launch of conv3x3_dgrad_f16x2_dense (weights packed once, dymax given) beside hipconv.conv3x3_dgrad on
the fp32 generic kernel AS THE f32 TRAINER CALLS IT (its per-call weight pack included), `iters` calls between one pair of
events, for the four layer shapes of tools/conv15h_bench.py, on gradients of magnitude 1e-4.

Prints two tables and one JSON line.  A tool: no test and no benchmark depends on it."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

NETS = {"simple15": ("simple", 0, 128), "resnet15x64": ("resnet", 1, 64), "resnet15x64x10": ("resnet", 10, 64),
        "resnet15x256": ("resnet", 1, 256), "resnet15x256x10": ("resnet", 10, 256)}
SHAPES = ((64, 64), (128, 64), (256, 128), (256, 256))      # (C of dy, C of dx): the data gradients of 64 -> 64 ... 256 -> 256
ARITHS = ("f16x2", "f32")


def stats(v, unit=1.0):
    return {"mean": round(unit * float(np.mean(v)), 3), "min": round(unit * float(np.min(v)), 3),
            "max": round(unit * float(np.max(v)), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="128,512")
    ap.add_argument("--nets", default=",".join(NETS))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--dgrad-iters", type=int, default=50)
    a = ap.parse_args()
    batches = [int(s) for s in a.batches.split(",")]
    nets = [s for s in a.nets.split(",") if s]
    import torch
    from alphapig_amd import hipconv, weights
    from alphapig_amd.train import HipTrainer

    rs = np.random.RandomState(31)
    step_rows = []
    print("%-16s %6s | %30s | %30s | %9s" % ("net", "batch", "f16x2 ms (min .. max)", "f32 ms (min .. max)", "f16x2/f32"))
    for name in nets:
        kind, blocks, nf = NETS[name]
        prm = weights.init_params(kind, 15, 15, 9, blocks, nf, seed=0, style="bench")
        for n in batches:
            states = (rs.rand(n, 9, 15, 15) < 0.2).astype(np.float32)
            pis = rs.dirichlet(np.ones(225), size=n).astype(np.float32)
            zs = rs.choice([-1.0, 1.0], size=n).astype(np.float32)
            trainers = {ar: HipTrainer(prm, kind, n_blocks=blocks, batch_size=n, seed=1, trunk_arith=ar) for ar in ARITHS}
            batch = {ar: tr.upload(states, pis, zs) for ar, tr in trainers.items()}
            ms = {ar: [] for ar in ARITHS}
            for rnd in range(a.rounds):
                for ar in ARITHS:
                    tr = trainers[ar]
                    for _ in range(a.warmup):
                        tr.train_step(batch[ar], None, None, 1e-3)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(a.iters):
                        tr.train_step(batch[ar], None, None, 1e-3)
                    torch.cuda.synchronize()
                    ms[ar].append(1e3 * (time.perf_counter() - t0) / a.iters)
            overflows = trainers["f16x2"].trunk_overflows
            for tr in trainers.values():
                tr.close()
            del trainers, batch
            torch.cuda.empty_cache()
            h, f = stats(ms["f16x2"]), stats(ms["f32"])
            step_rows.append({"net": name, "batch": n, "f16x2_ms": h, "f32_ms": f, "ratio": round(h["mean"] / f["mean"], 3),
                              "trunk_overflows": int(overflows)})
            print("%-16s %6d | %10.2f (%7.2f .. %7.2f) | %10.2f (%7.2f .. %7.2f) | %9.3f%s" % (
                name, n, h["mean"], h["min"], h["max"], f["mean"], f["min"], f["max"], h["mean"] / f["mean"],
                "  (%d overflows)" % overflows if overflows else ""))

    dgrad_rows = []
    print("%-12s %6s | %30s | %30s | %9s" % ("dgrad", "boards", "f16x2 us (min .. max)", "f32 us (min .. max)", "f32/f16x2"))
    g = torch.Generator().manual_seed(5)
    for c_dy, c_dx in SHAPES:
        w = (torch.randn(c_dy, c_dx, 3, 3, generator=g) / (9.0 * c_dy) ** 0.5).cuda()
        packed = hipconv.conv15h_pack_many([(w, None)])[0]
        flag = torch.zeros(1, dtype=torch.int32, device="cuda")
        for n in batches:
            dy = (torch.randn(n, c_dy, 15, 15, generator=g) * 1e-4).cuda()
            dymax = dy.abs().amax(dim=(0, 2, 3)).reshape(1, -1).contiguous()
            calls = {"f16x2": lambda: hipconv.conv3x3_dgrad_f16x2_dense(dy, packed[1], dymax, flag),
                     "f32": lambda: hipconv.conv3x3_dgrad(dy, w, hipconv.DENSE)}
            us = {ar: [] for ar in ARITHS}
            for rnd in range(a.rounds):
                for ar in ARITHS:
                    for _ in range(a.warmup):
                        calls[ar]()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(a.dgrad_iters):
                        calls[ar]()
                    e1.record()
                    e1.synchronize()
                    us[ar].append(1e3 * e0.elapsed_time(e1) / a.dgrad_iters)
            assert int(flag.item()) == 0
            h, f = stats(us["f16x2"]), stats(us["f32"])
            dgrad_rows.append({"shape": "%d -> %d" % (c_dy, c_dx), "boards": n, "f16x2_us": h, "f32_us": f,
                               "speedup": round(f["mean"] / h["mean"], 3)})
            print("%-12s %6d | %10.1f (%7.1f .. %7.1f) | %10.1f (%7.1f .. %7.1f) | %9.2f" % (
                "%d -> %d" % (c_dy, c_dx), n, h["mean"], h["min"], h["max"], f["mean"], f["min"], f["max"], f["mean"] / h["mean"]))
    print(json.dumps({"generic_train_bench": {"steps": step_rows, "dgrad": dgrad_rows}, "rounds": a.rounds, "iters": a.iters,
                      "warmup": a.warmup, "dgrad_iters": a.dgrad_iters}))


if __name__ == "__main__":
    main()
