#!/usr/bin/env python3
"""Which kernels a forward launches, as a trace that two source trees can be compared by.

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/route_trace.py     (on the GPU, once per tree)
    python tools/route_trace.py --compare A_kernel_trace.csv B_kernel_trace.csv            (on the host)
    python tools/route_trace.py --compare --whole A_kernel_trace.csv B_kernel_trace.csv    (traces of any other run)
    ... --rename OLD=NEW (repeatable): kernel OLD of trace A counts as NEW, the name it has in B -- names without arguments
    and without a template's "void " in front, as tools/device_code_diff.py --rename takes them

Bits cannot tell the small-batch trunk kernels from the batched ones (they are bit-equal by contract); the launch sequence
can.  The run makes one forward per case below: every engine of tests/test_gpu_forward_modes.py at 5 and at 40 boards, every
apz_test_select_trunk kind, APZ_F16X2_K8=1, a calibrated engine with nonzero exponents, and an overflowing batch with the
automatic response on.  In front of forward k and behind it the run launches the root sampler on k + 1 rows: --compare cuts
the trace at those launches and compares, case by case (the run prints their numbers), the sequence of (kernel, grid,
workgroup, LDS bytes) between them.  The runtime's own copy kernels are left out: whether a hipMemcpyAsync becomes such a
kernel or a DMA transfer is its choice from run to run (its fill kernels, the ticket resets, stay in).  Exit status 1 on any
difference.  --whole: the traces have no separator launches (tools/train_digest.py under rocprofv3): each is one case, compared
from its first launch to its last."""
import csv
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

SEPARATOR = "root_sample_kernel"


def cases():
    """-> [(label, make() -> net, boards)]"""
    import numpy as np
    from alphapig_amd.policy_value_net import PolicyValueNet
    import test_gpu_forward_modes as fm

    def select(name, kind):
        def make():
            net = fm._make(name)
            net._ck(net.L.apz_test_select_trunk(net._h, kind))
            return net
        return make

    def k8():
        os.environ["APZ_F16X2_K8"] = "1"
        try:
            return fm._make("f16x2")
        finally:
            del os.environ["APZ_F16X2_K8"]

    def calibrated(name):
        def make():
            net = PolicyValueNet(15, 15, batch_size=64, n_blocks=2, n_filter=128, model_params=fm._big(), trunk_arith="f16x2",
                                 uniform_trunk=name == "f16x2-uniform")
            net.calibrate_trunk(fm._positions(15)[1][:40])
            assert any(net.trunk_act_exponents())
            return net
        return make

    def overflowing():
        net = fm._make("f16x2")
        net.set_params(fm._big())
        net.set_act_scale_auto(True)
        return net

    out = [("%s n=%d" % (name, n), lambda name=name: fm._make(name), n) for name, n, graphs in fm.CASES if not graphs]
    # apz_test_select_trunk: 0 direct, 3 Winograd (the default), 4 batched at every size, 5 ... and no quarter items
    out += [("%s select=%d n=%d" % (name, kind, n), select(name, kind), n)
            for name in ("f32", "f16x2-uniform") for kind in (0, 3, 4, 5) for n in (5, 40)]
    out += [("APZ_F16X2_K8 n=%d" % n, k8, n) for n in (5, 40)]
    out += [("calibrated %s n=%d" % (name, n), calibrated(name), n) for name in ("f16x2", "f16x2-uniform") for n in (5, 40)]
    out += [("overflow, act_scale auto n=40", overflowing, 40)]
    return out, fm, np


def run():
    todo, fm, np = cases()
    for k, (label, make, n) in enumerate(todo):
        net = make()
        try:
            planes = fm._positions(net.board_width)[1][:n]
            mark = lambda: net.sample_moves(np.ones((k + 1, net.hw), np.int32))
            mark()
            net.forward_with_logits(planes)
            mark()
        finally:
            net.close()
        print("%3d %s" % (k, label), flush=True)


def forwards(path, whole=False, renames=None):
    """kernel-trace CSV -> {case + 1: [(kernel, grid, workgroup, LDS)] between the case's two sampler launches}
    (whole: {1: every launch of the trace}; renames: see --rename, None = names as the trace has them)"""
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Dispatch_Id"]))

    def name(r):
        n = r["Kernel_Name"].split("(")[0]
        if renames is None:
            return n
        n = n[5:] if n.startswith("void ") else n
        return renames.get(n, n)
    shape = lambda r: (name(r),) + tuple(
        int(r[c + a]) for c in ("Grid_Size_", "Workgroup_Size_") for a in "XYZ") + (int(r["LDS_Block_Size"]),)
    out, cur = ({1: []}, None) if whole else ({}, None)
    if whole:
        cur = out[1]
    for r in rows:
        s = shape(r)
        if s[0].startswith("__amd_rocclr_copy"):
            continue
        if SEPARATOR in s[0] and not whole:
            cur = out.setdefault(s[1] // s[4], []) if cur is None else None     # (one 64-thread workgroup per row)
        elif cur is not None:
            cur.append(s)
    return out


def compare(a, b, whole=False, renames=None):
    fa, fb = forwards(a, whole, renames), forwards(b, whole, renames and {})
    bad = 0
    for k in sorted(set(fa) | set(fb)):
        same = fa.get(k) == fb.get(k)
        bad += not same
        print("%-9s case %3d: %d launches" % ("identical" if same else "DIFFERENT", k - 1, len(fa.get(k, ()))))
        if not same:
            for x, y in zip(fa.get(k, ()), fb.get(k, ())):
                if x != y:
                    print("    A %s\n    B %s" % (x, y))
                    break
    print("forwards: %d in A, %d in B, %d different" % (len(fa), len(fb), bad))
    return 1 if bad or not fa else 0


if __name__ == "__main__":
    if "--compare" in sys.argv:
        i = sys.argv.index("--compare")
        rest = sys.argv[i + 1:]
        pairs = [rest[j + 1].split("=", 1) for j, a in enumerate(rest[:-1]) if a == "--rename"]
        paths = [a for j, a in enumerate(rest) if a not in ("--whole", "--rename") and (j == 0 or rest[j - 1] != "--rename")]
        sys.exit(compare(paths[0], paths[1], "--whole" in sys.argv, dict(pairs) or None))
    run()
