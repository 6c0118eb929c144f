#!/usr/bin/env python3
"""What the legal-move policy costs in the evaluator (apz_set_legal_policy): the 10-block / 128-filter residual net at 15x15,
switch off and on ALTERNATING round after round in ONE process, at 1, 32 and 512 boards.

    python tools/legal_policy_bench.py [--rounds 5] [--iters 40] [--warmup 10] [--blocks 10] [--arith auto]

Per case two figures, each the mean of the per-round medians / means with their spread:
  forward   one slot submission (apz_submit_codes) between two HIP events on the engine's stream, waited for before the
            next: launch gaps included, the host copies of submit / wait excluded.  The codes sit in the slot's pinned host
            buffer; with the switch on the head reads them there a second time (the stem read them first).
  head_fc   apz_kernel_time_ms(APZ_K_HEAD_FC) per forward, from a pass of its own with apz_set_profiling(1): the policy
            FullyConnected launch and the softmax / value launch (and, in the planes rows, the occupancy launch).
"planes" rows (512 boards): apz_forward on planes in device memory -- the occupancy is staged by occupancy_planes_kernel
in front of the head.  The switch-off runs launch exactly what the engine launched before the switch existed.

Prints a table and one JSON line.  A tool: no test and no benchmark depends on it."""
import argparse
import json
import os
import sys

import numpy as np

SIZES = (1, 32, 512)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--blocks", type=int, default=10)
    ap.add_argument("--arith", default="auto")
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    from alphapig_amd import weights
    from alphapig_amd.policy_value_net import PolicyValueNet
    from alphapig_amd.treepool import TreePool

    prm = weights.init_params("resnet", 15, 15, 9, a.blocks, 128, seed=0, style="bench")
    net = PolicyValueNet(15, 15, batch_size=512, n_blocks=a.blocks, n_filter=128, model_params=prm, trunk_arith=a.arith)
    stream = torch.cuda.ExternalStream(net.L.apz_stream(net._h))
    pool = TreePool(15, 15, 5, n_games=1, n_playout=1)
    rs = np.random.RandomState(3)
    codes = []
    for _ in range(512):
        k = int(rs.randint(0, 121))
        pool.set_position(0, rs.permutation(225)[:k], [1 + (i % 2) for i in range(k)], 1 + (k % 2))
        codes.append(pool.codes(0))
    codes = np.stack(codes)
    planes = torch.as_tensor(pool.codes_to_planes(codes, 9)).cuda()
    out_p, out_v = torch.empty((512, 225), device="cuda"), torch.empty((512,), device="cuda")
    pool.close()
    torch.cuda.synchronize()

    def slot(n, queued=lambda: None):
        k = net.submit_codes_slot(0, codes[:n])
        queued()
        net.wait_slot(0, k)

    def dev_planes(n, queued=lambda: None):
        # (APZ_ARITH_F16X2: apz_forward returns with the stream drained, so the second event closes an idle stream)
        net._ck(net.L.apz_forward(net._h, planes.data_ptr(), n, out_p.data_ptr(), out_v.data_ptr(), None, None))
        queued()
        net.sync()

    def timed(run, n):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(stream)
        run(n, lambda: t1.record(stream))
        t1.synchronize()
        return t0.elapsed_time(t1)

    cases = [("slot", slot, n) for n in SIZES] + [("planes", dev_planes, 512)]
    fwd = {(e, n, on): [] for e, _, n in cases for on in (0, 1)}
    head = {k: [] for k in fwd}
    for rnd in range(a.rounds):
        for entry, run, n in cases:
            for on in (0, 1):
                net.set_legal_policy(on)
                for _ in range(a.warmup):
                    run(n)
                fwd[(entry, n, on)].append(1e3 * float(np.median([timed(run, n) for _ in range(a.iters)])))
                net.set_profiling(1)
                for _ in range(a.iters):
                    run(n)
                net.sync()
                head[(entry, n, on)].append(1e3 * net.kernel_time_ms("head_fc")[0] / a.iters)
                net.set_profiling(0)
    assert net.trunk_overflows() == 0
    net.close()
    rows = []
    for entry, _, n in cases:
        r = {"entry": entry, "boards": n, "blocks": a.blocks, "arith": a.arith}
        for name, per in (("forward", fwd), ("head_fc", head)):
            off, on = per[(entry, n, 0)], per[(entry, n, 1)]
            r[name] = {"off_us": round(float(np.mean(off)), 2), "off_runs": [round(x, 2) for x in off],
                       "on_us": round(float(np.mean(on)), 2), "on_runs": [round(x, 2) for x in on],
                       "ratio": round(float(np.mean(on)) / float(np.mean(off)), 4)}
        rows.append(r)
    print("%-6s %6s | %-44s | %s" % ("entry", "boards", "forward us: off (min .. max)  on (min .. max)  on / off",
                                    "head_fc us: off (min .. max)  on (min .. max)  on / off"))
    for r in rows:
        cell = lambda d: "%8.1f (%7.1f .. %7.1f) %8.1f (%7.1f .. %7.1f) %6.3f" % (
            d["off_us"], min(d["off_runs"]), max(d["off_runs"]), d["on_us"], min(d["on_runs"]), max(d["on_runs"]), d["ratio"])
        print("%-6s %6d | %s | %s" % (r["entry"], r["boards"], cell(r["forward"]), cell(r["head_fc"])))
    print(json.dumps({"legal_policy_bench": rows, "rounds": a.rounds, "iters": a.iters, "warmup": a.warmup}))


if __name__ == "__main__":
    main()
