#!/usr/bin/env python3
"""conv15h_kernel (csrc/conv15_split.h, trunk_arith="f16x2") against the fp32 generic kernel (csrc/conv3x3_mfma.h,
trunk_arith="f32") on the 15x15 nets that have no Winograd trunk, in ONE process, the two arithmetics ALTERNATING round after
round so that clock and temperature drift falls on both alike.

    python tools/conv15h_bench.py [--batches 1,32,128,512] [--forward-batches 1,32,512] [--rounds 5] [--iters 50] [--warmup 10]

Layers: the simple net holds all four shapes -- 64 -> 64 (layer 1), 64 -> 128 (2), 128 -> 256 (4), 256 -> 256 (5).  One
measurement is apz_conv3x3_bench: `iters` launches of the layer on its real input (the activations of random planes, not
zeros: the clock a matrix kernel holds depends on its data) between one pair of events, after `warmup` untimed launches.
Whole forwards: the 256-filter residual net with ten blocks and the simple net; `iters` forwards queued by apz_prewarm under
apz_set_profiling(1), the "trunk" class (every 3x3 layer behind the first) and the "forward" class read back with
apz_kernel_time_ms.  Reported: mean over the rounds and the spread of the per-round means (min .. max), and f32 / f16x2.

Prints two tables and one JSON line.  A tool: no test and no benchmark depends on it."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

LAYERS = ((1, "64 -> 64"), (2, "64 -> 128"), (4, "128 -> 256"), (5, "256 -> 256"))
ARITHS = ("f16x2", "f32")


def stats(v):
    return {"us": round(1e3 * float(np.mean(v)), 2), "us_min": round(1e3 * float(np.min(v)), 2),
            "us_max": round(1e3 * float(np.max(v)), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,32,128,512")
    ap.add_argument("--forward-batches", default="1,32,512")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--blocks", type=int, default=10)
    a = ap.parse_args()
    batches = [int(s) for s in a.batches.split(",")]
    fbatches = [int(s) for s in a.forward_batches.split(",")]
    cap = max(batches + fbatches)
    from alphapig_amd import weights
    from alphapig_amd.policy_value_net import PolicyValueNet

    planes = (np.random.RandomState(31).rand(cap, 9, 15, 15) < 0.2).astype(np.float32)
    nets = {"simple15": ("simple", 0, 128), "resnet15x256": ("resnet", a.blocks, 256)}
    engines = {}
    for name, (kind, blocks, nf) in nets.items():
        prm = weights.init_params(kind, 15, 15, 9, blocks, nf, seed=0, style="bench")
        for arith in ARITHS:
            engines[(name, arith)] = PolicyValueNet(15, 15, batch_size=cap, n_blocks=blocks, n_filter=nf, model_params=prm,
                                                    net_kind=kind, trunk_arith=arith)

    layer_ms = {(l, n, arith): [] for l, _ in LAYERS for n in batches for arith in ARITHS}
    for n in batches:
        for arith in ARITHS:                                # the layer bench reads the planes of the last forward
            engines[("simple15", arith)].forward_planes(planes[:n])
        for rnd in range(a.rounds):
            for l, _ in LAYERS:
                for arith in ARITHS:
                    layer_ms[(l, n, arith)].append(engines[("simple15", arith)].conv_bench(l, n, a.iters, a.warmup))
    fwd_ms = {(name, n, arith, cls): [] for name in nets for n in fbatches for arith in ARITHS for cls in ("trunk", "forward")}
    for rnd in range(a.rounds):
        for name in nets:
            for n in fbatches:
                for arith in ARITHS:
                    net = engines[(name, arith)]
                    net.prewarm(n, a.warmup)
                    net.set_profiling(1)                    # (synchronises and zeroes the sums)
                    net.prewarm(n, a.iters)
                    net.sync()
                    for cls in ("trunk", "forward"):
                        fwd_ms[(name, n, arith, cls)].append(net.kernel_time_ms(cls)[0] / a.iters)
                    net.set_profiling(0)
    for key, net in engines.items():
        assert net.trunk_overflows() == 0, key
        net.close()

    layer_rows, fwd_rows = [], []
    print("%-12s %6s | %28s | %28s | %9s" % ("layer", "boards", "f16x2 us (min .. max)", "f32 us (min .. max)", "f32/f16x2"))
    for l, shape in LAYERS:
        for n in batches:
            h, f = stats(layer_ms[(l, n, "f16x2")]), stats(layer_ms[(l, n, "f32")])
            layer_rows.append({"layer": shape, "boards": n, "f16x2": h, "f32": f, "speedup": round(f["us"] / h["us"], 3)})
            print("%-12s %6d | %9.1f (%7.1f .. %7.1f) | %9.1f (%7.1f .. %7.1f) | %9.2f" % (
                shape, n, h["us"], h["us_min"], h["us_max"], f["us"], f["us_min"], f["us_max"], f["us"] / h["us"]))
    print("%-12s %6s %8s | %28s | %28s | %9s" % ("net", "boards", "class", "f16x2 us (min .. max)", "f32 us (min .. max)", "f32/f16x2"))
    for name in nets:
        for n in fbatches:
            for cls in ("trunk", "forward"):
                h, f = stats(fwd_ms[(name, n, "f16x2", cls)]), stats(fwd_ms[(name, n, "f32", cls)])
                fwd_rows.append({"net": name, "boards": n, "class": cls, "f16x2": h, "f32": f, "speedup": round(f["us"] / h["us"], 3)})
                print("%-12s %6d %8s | %9.1f (%7.1f .. %7.1f) | %9.1f (%7.1f .. %7.1f) | %9.2f" % (
                    name, n, cls, h["us"], h["us_min"], h["us_max"], f["us"], f["us_min"], f["us_max"], f["us"] / h["us"]))
    print(json.dumps({"conv15h_bench": {"layers": layer_rows, "forwards": fwd_rows}, "rounds": a.rounds, "iters": a.iters,
                      "warmup": a.warmup, "blocks": a.blocks}))


if __name__ == "__main__":
    main()
