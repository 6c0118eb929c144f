#!/usr/bin/env python3
"""sha256 digests of what the training step computes, for comparing two source trees bit by bit (on the GPU):

    python tools/train_digest.py > digest.txt          (once per tree; diff the two files)

Per case three train_steps, then one digest each over the parameters (moving statistics included), Adam's moments and the
last step's gradients, every tensor in name order; the step's (loss, entropy) pairs are printed as float hex.  Cases: the
15x15 resnet (2 blocks, 128 filters, n = 6) in both trunk arithmetics, the 8x8 resnet (1 block, 64 filters, n = 4: the dense
residual path), the 8x8 simple net (n = 4), one f16x2 step that overflows and is repeated exactly (bnA1_gamma of one
channel at 5e3, n = 40), and one policy_update each on a list mini-batch and on a DeviceBatch.  Behind those, the guard
and the average: guarded f32, guarded f32 with a clip_norm that clips, a guarded step that is skipped (NaN z) between two
good ones, the overflowing step guarded, ema_decay on in both arithmetics, framed boards of side 6 and 14, legal_policy at
15x15 and 8x8 (the states are random planes: about two cells in three count as occupied), and a state() -> fresh trainer ->
load_state() -> one more step round trip with guard and average on.  Every case also prints its counters
and the guard's three last_* values, and the averaged weights' digest where they exist.  The tests "the same bits on
every run" are what makes the comparison meaningful.  The same run under rocprofv3 --kernel-trace is the launch sequence
that tools/route_trace.py --compare --whole compares."""
import hashlib
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from alphapig_amd import weights  # noqa: E402
from alphapig_amd.train import DeviceBatch, HipTrainer, policy_update  # noqa: E402


def problem(kind, side, n, blocks, filters, seed):
    rs = np.random.RandomState(seed)
    prm = weights.init_params(kind, side, side, 9, blocks, filters, seed=seed + 1, style="bench")
    states = (rs.rand(n, 9, side, side) > 0.6).astype(np.float32)
    pis = rs.dirichlet(np.ones(side * side), size=n).astype(np.float32)
    zs = rs.choice([-1.0, 1.0], size=n).astype(np.float32)
    return prm, states, pis, zs


def digest(arrays):
    h = hashlib.sha256()
    for k in sorted(arrays):
        a = np.ascontiguousarray(arrays[k])
        h.update(("%s %s %s;" % (k, a.dtype, a.shape)).encode())
        h.update(a.tobytes())
    return h.hexdigest()


def report(label, tr, results):
    host = lambda group: {k: v.cpu().numpy() for k, v in group.items()}
    print("%s: t %d, overflows %d" % (label, tr.t, tr.trunk_overflows))
    print("  results  %s" % " ".join("(%s)" % ", ".join(float(x).hex() for x in r) for r in results))
    print("  params   %s" % digest(tr.get_params()))
    print("  m        %s" % digest(host(tr.m)))
    print("  v        %s" % digest(host(tr.v)))
    print("  grads    %s" % digest(tr.get_grads()))
    if tr.ema_p is not None:
        print("  ema_p    %s" % digest(tr.ema_params()))
    fhex = lambda x: None if x is None else float(x).hex()
    print("  counters skipped %d clipped %d ema_updates %d; last grad_norm %s rescale_eff %s skip_reason %r" %
          (tr.skipped_steps, tr.clipped_steps, tr.ema_updates, fhex(tr.last_grad_norm), fhex(tr.last_rescale_eff),
           tr.last_skip_reason), flush=True)


def steps(label, kind, side, n, blocks, filters, seed, count=3, hot=False, bad=(), **kw):
    """bad: the steps (from 0) whose mini-batch has a NaN z"""
    prm, states, pis, zs = problem(kind, side, n, blocks, filters, seed)
    nan_zs = zs.copy()
    nan_zs[1] = np.nan
    if hot:
        prm = dict(prm)
        prm["bnA1_gamma"] = np.array(prm["bnA1_gamma"], dtype=np.float32).copy()
        prm["bnA1_gamma"][3] = 5e3
    tr = HipTrainer(prm, kind, n_blocks=blocks, batch_size=n, dropout=0.5, seed=2, **kw)
    results = [tr.train_step(states, pis, nan_zs if i in bad else zs, 1e-3) for i in range(count)]
    assert tr.skipped_steps == len(bad), "the guard did not refuse exactly the NaN steps"
    if kw.get("clip_norm"):
        assert tr.clipped_steps > 0, "clip_norm %r clipped no step" % kw["clip_norm"]
    if hot:
        assert tr.trunk_overflows == 1, "the hot channel did not raise the overflow word"
    report(label, tr, results)
    tr.close()


def updates():
    prm, states, pis, zs = problem("resnet", 15, 6, 2, 128, seed=31)
    for label, device in (("policy_update, list mini-batch", False), ("policy_update, DeviceBatch", True)):
        tr = HipTrainer(prm, "resnet", n_blocks=2, batch_size=6, dropout=0.5, seed=2)
        batch = tr.upload(states, pis, zs) if device else [(states[i], pis[i], float(zs[i])) for i in range(len(zs))]
        assert isinstance(batch, DeviceBatch) == device
        mon = {}
        res = policy_update(tr, batch, learn_rate=2e-3, lr_multiplier=1.0, epochs=3, kl_targ=0.02, monitors=mon)
        report(label, tr, [res, tuple(mon[k] for k in sorted(mon))])
        tr.close()


def round_trip():
    """two steps, state() into a fresh trainer built from other weights, one more step there"""
    prm, states, pis, zs = problem("resnet", 15, 6, 2, 128, seed=41)
    other = problem("resnet", 15, 6, 2, 128, seed=42)[0]
    kw = dict(n_blocks=2, batch_size=6, dropout=0.5, seed=2, step_guard=True, ema_decay=0.9)
    a, b = HipTrainer(prm, "resnet", **kw), HipTrainer(other, "resnet", **kw)
    results = [a.train_step(states, pis, zs, 1e-3) for _ in range(2)]
    b.load_state(a.state())
    results.append(b.train_step(states, pis, zs, 1e-3))
    report("state round trip, guarded with the average", b, results)
    a.close()
    b.close()


def main():
    steps("resnet 15x15 2x128 n=6 f32", "resnet", 15, 6, 2, 128, seed=11)
    steps("resnet 15x15 2x128 n=6 f16x2", "resnet", 15, 6, 2, 128, seed=11, trunk_arith="f16x2")
    steps("resnet 8x8 1x64 n=4", "resnet", 8, 4, 1, 64, seed=12)
    steps("simple 8x8 n=4", "simple", 8, 4, 0, 128, seed=13)
    steps("resnet 15x15 2x128 n=40 f16x2, overflowed step", "resnet", 15, 40, 2, 128, seed=21, count=1, hot=True,
          trunk_arith="f16x2")
    updates()
    steps("guarded f32", "resnet", 15, 6, 2, 128, seed=11, step_guard=True)
    steps("guarded f32, clip_norm 1e-3", "resnet", 15, 6, 2, 128, seed=11, clip_norm=1e-3)
    steps("guarded f32, step 1 skipped", "resnet", 15, 6, 2, 128, seed=11, bad=(1,), step_guard=True)
    steps("guarded f16x2, overflowed step", "resnet", 15, 40, 2, 128, seed=21, count=1, hot=True, trunk_arith="f16x2",
          step_guard=True)
    steps("average f32", "resnet", 15, 6, 2, 128, seed=11, ema_decay=0.9)
    steps("average f16x2", "resnet", 15, 6, 2, 128, seed=11, trunk_arith="f16x2", ema_decay=0.9)
    steps("framed 6x6 2x128 n=6", "resnet", 6, 6, 2, 128, seed=14, framed=True)
    steps("framed 14x14 2x128 n=6", "resnet", 14, 6, 2, 128, seed=15, framed=True)
    steps("legal_policy 15x15 2x128 n=6", "resnet", 15, 6, 2, 128, seed=16, legal_policy=True)
    steps("legal_policy 8x8 1x64 n=4", "resnet", 8, 4, 1, 64, seed=17, legal_policy=True)
    round_trip()


if __name__ == "__main__":
    main()
