#!/usr/bin/env python3
"""What a leaf symmetry costs: one slot submission (apz_submit_codes: the expand kernel, the forward, the fold kernel)
between two HIP events on the engine's stream, on the 10-block / 128-filter residual net at 15x15, in ONE process.

    python tools/leaf_sym_bench.py [--rounds 5] [--iters 40] [--warmup 10] [--blocks 10] [--arith auto] [--tree DIR]

Cases: "none" and "keyed" at 1, 32 and 512 positions; "mean8" at 1 and 64 positions, beside "none" at the 8 and 512 boards
those forwards really run.  One engine serves them all (max_batch 512); the cases are measured ALTERNATING, round after
round, so that clock and temperature drift falls on all of them alike.  A measurement is the median over `iters`
submissions of random positions, each waited for before the next (the latency a caller of the slot interface sees on the
GPU side: launch gaps between the forward's kernels included, the host copies of submit / wait excluded); reported is the
mean of the per-round medians with their spread, and the difference to the "none" case it stands beside.

--tree DIR: import alphapig_amd from DIR (a built checkout of another commit) and measure the "none" cases only -- the
figures of a commit that has no leaf symmetry, from the same box and the same tool.

Prints a table and one JSON line.  A tool: no test and no benchmark depends on it."""
import argparse
import json
import os
import sys

import numpy as np

# (mode, positions, the "none" case it is compared with: boards of that forward)
CASES = [("none", 1, None), ("keyed", 1, 1), ("none", 8, None), ("mean8", 1, 8), ("none", 32, None), ("keyed", 32, 32),
         ("none", 512, None), ("keyed", 512, 512), ("mean8", 64, 512)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--blocks", type=int, default=10)
    ap.add_argument("--arith", default="auto")
    ap.add_argument("--tree", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree) if a.tree else os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    from alphapig_amd import weights
    from alphapig_amd.policy_value_net import PolicyValueNet
    from alphapig_amd.treepool import TreePool

    cases = [c for c in CASES if c[0] == "none"] if a.tree else CASES
    prm = weights.init_params("resnet", 15, 15, 9, a.blocks, 128, seed=0, style="bench")
    net = PolicyValueNet(15, 15, batch_size=512, n_blocks=a.blocks, n_filter=128, model_params=prm, trunk_arith=a.arith)
    stream = torch.cuda.ExternalStream(net.L.apz_stream(net._h))
    pool = TreePool(15, 15, 5, n_games=1, n_playout=1)
    rs = np.random.RandomState(3)
    codes = []
    for _ in range(512):
        k = int(rs.randint(0, 81))
        pool.set_position(0, rs.permutation(225)[:k], [1 + (i % 2) for i in range(k)], 1 + (k % 2))
        codes.append(pool.codes(0))
    codes = np.stack(codes)
    pool.close()

    def one(n):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(stream)
        k = net.submit_codes_slot(0, codes[:n])
        t1.record(stream)
        net.wait_slot(0, k)
        t1.synchronize()
        return t0.elapsed_time(t1)

    per = {c[:2]: [] for c in cases}
    for rnd in range(a.rounds):
        for mode, n, _ in cases:
            if not a.tree:
                net.set_leaf_symmetry(mode, 1234)
            for _ in range(a.warmup):
                one(n)
            per[(mode, n)].append(float(np.median([one(n) for _ in range(a.iters)])))
    assert net.trunk_overflows() == 0
    net.close()
    rows = []
    for mode, n, beside in cases:
        v = per[(mode, n)]
        r = {"mode": mode, "positions": n, "boards": n * (8 if mode == "mean8" else 1), "blocks": a.blocks, "arith": a.arith,
             "us": round(1e3 * float(np.mean(v)), 2), "us_min": round(1e3 * float(np.min(v)), 2),
             "us_max": round(1e3 * float(np.max(v)), 2)}
        if beside is not None:
            r["over_none_us"] = round(1e3 * (float(np.mean(v)) - float(np.mean(per[("none", beside)]))), 2)
        rows.append(r)
    print("%-6s %9s %6s | %30s | %s" % ("mode", "positions", "boards", "submission us (min .. max)", "over none at these boards, us"))
    for r in rows:
        print("%-6s %9d %6d | %10.1f (%8.1f .. %8.1f) | %s" % (r["mode"], r["positions"], r["boards"], r["us"], r["us_min"],
                                                               r["us_max"], r.get("over_none_us", "")))
    print(json.dumps({"leaf_sym_bench": rows, "rounds": a.rounds, "iters": a.iters, "warmup": a.warmup,
                      "tree": a.tree or "this"}))


if __name__ == "__main__":
    main()
