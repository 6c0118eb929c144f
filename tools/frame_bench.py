#!/usr/bin/env python3
"""What a framed board costs: forwards of 512 boards and of 1 board on the 10-block / 128-filter residual net at 15x15
(the kernels' own size) and at 13x13 and 9x9 (framed on the same kernels, csrc/frame15.h), in ONE process.

    python tools/frame_bench.py [--sizes 15,13,9] [--batches 512,1] [--rounds 5] [--iters 100] [--warmup 20] [--blocks 10]

For each arithmetic ("f16x2", "f32") one engine per size is created; the sizes are then measured ALTERNATING, round after
round, so that clock and temperature drift falls on all of them alike.  A measurement is `iters` forwards of empty
boards queued by apz_prewarm (no host copies, no synchronisation between them) under apz_set_profiling(1), after
`warmup` untimed ones: HIP events around the trunk class (all trunk convolutions of a forward and, on a framed engine,
their clears) and around the whole forward.  Reported per forward, mean over the rounds with the spread (min .. max of
the per-round means), and relative to the 15x15 engine of the same process and arithmetic.

At one board "f16x2" engines run the exact-fp32 small-batch kernel ("which arithmetic a batch gets"), so the
two arithmetics differ at 512 boards only.  A framed forward has one launch more in front of the stem (the framing
kernel) and one clear behind every layer but the last: the one-board rows show what these launches cost.

Prints a table and one JSON line.  A tool: no test and no benchmark depends on it."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="15,13,9")
    ap.add_argument("--batches", default="512,1")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=10)
    ap.add_argument("--ariths", default="f16x2,f32")
    a = ap.parse_args()
    sizes = [int(s) for s in a.sizes.split(",")]
    batches = [int(s) for s in a.batches.split(",")]
    from alphapig_amd import weights
    from alphapig_amd.policy_value_net import PolicyValueNet

    rows = []
    for arith in a.ariths.split(","):
        nets = {}
        for s in sizes:
            prm = weights.init_params("resnet", s, s, 9, a.blocks, 128, seed=0, style="bench")
            nets[s] = PolicyValueNet(s, s, batch_size=max(batches), n_blocks=a.blocks, n_filter=128, model_params=prm,
                                     trunk_arith=arith)
        per = {(s, n): {"trunk": [], "forward": []} for s in sizes for n in batches}
        for rnd in range(a.rounds):
            for n in batches:
                for s in sizes:                         # alternating: every size once per round and batch
                    net = nets[s]
                    net.prewarm(n, a.warmup)
                    net.set_profiling(1)                # (synchronises and zeroes the sums)
                    net.prewarm(n, a.iters)
                    net.sync()
                    for cls in ("trunk", "forward"):
                        ms, cnt = net.kernel_time_ms(cls)
                        per[(s, n)][cls].append(ms / a.iters)
                    net.set_profiling(0)
        for s in sizes:
            assert nets[s].trunk_overflows() == 0
            nets[s].close()
        for n in batches:
            base = {cls: float(np.mean(per[(sizes[0], n)][cls])) for cls in ("trunk", "forward")}
            for s in sizes:
                r = {"arith": arith, "side": s, "boards": n, "blocks": a.blocks}
                for cls in ("trunk", "forward"):
                    v = per[(s, n)][cls]
                    r[cls + "_us"] = round(1e3 * float(np.mean(v)), 2)
                    r[cls + "_us_min"] = round(1e3 * float(np.min(v)), 2)
                    r[cls + "_us_max"] = round(1e3 * float(np.max(v)), 2)
                    r[cls + "_vs_%d" % sizes[0]] = round(float(np.mean(v)) / base[cls], 4)
                rows.append(r)
    ref = sizes[0]
    print("%-6s %5s %6s | %26s %8s | %26s %8s" % ("arith", "side", "boards", "trunk us (min .. max)", "vs %d" % ref,
                                                   "forward us (min .. max)", "vs %d" % ref))
    for r in rows:
        print("%-6s %5d %6d | %9.1f (%7.1f .. %7.1f) %8.3f | %9.1f (%7.1f .. %7.1f) %8.3f" % (
            r["arith"], r["side"], r["boards"], r["trunk_us"], r["trunk_us_min"], r["trunk_us_max"], r["trunk_vs_%d" % ref],
            r["forward_us"], r["forward_us_min"], r["forward_us_max"], r["forward_vs_%d" % ref]))
    print(json.dumps({"frame_bench": rows, "rounds": a.rounds, "iters": a.iters, "warmup": a.warmup}))


if __name__ == "__main__":
    main()
