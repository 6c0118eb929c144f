#!/usr/bin/env python3
"""Compare the gfx950 device code of apz_engine.hip between two source trees, kernel by kernel.

    tools/device_code_diff.py <tree A> <tree B> [--keep DIR] [--rename OLD=NEW ...]

A tree is a checkout (or an export of one) with alphapig_amd/csrc and include/, or the a.s / b.s that an earlier run left
under --keep.  Each tree's apz_engine.hip is compiled
device-only to assembly with the flags of alphapig_amd/build.py; comments and directives are dropped and every kernel gets
one verdict:
    identical    the same lines (basic-block labels compared without the function's index in the module)
    scalar-only  the same number of instructions and the same count per mnemonic, the same sequence of non-scalar
                 instructions once SGPR operands are masked, and the same resource metadata (registers, spills, LDS, scratch)
    different    anything else, a kernel that exists on one side only included
--rename OLD=NEW (repeatable): kernel OLD of tree A is compared with kernel NEW of tree B and listed as "OLD -> NEW", instead
of one gone and one added.  Both are demangled names without arguments and without a template's "void " in front, e.g.
apz::bn_stats_r16_kernel='apz::bn_stats_rows_kernel<apz::Board15>'.
Exit status 1 if any kernel is "different".  CPU only: nothing here runs a kernel.
"""
import collections
import os
import re
import subprocess
import sys
import tempfile

FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-Wall", "-Wno-unused-result"]
META = ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "group_segment_fixed_size",
        "private_segment_fixed_size")
SGPR = re.compile(r"\bs(\d+|\[\d+:\d+\])")
LOCAL_LABEL = re.compile(r"\.LBB\d+_(\d+)")


def assemble(tree, out):
    if os.path.isfile(tree):                                        # an assembly file kept from an earlier run (--keep)
        return tree
    csrc = os.path.join(tree, "alphapig_amd", "csrc")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc] + FLAGS + ["-I" + os.path.join(tree, "include"), "-I" + csrc, "--offload-device-only", "-S",
                                      os.path.join(csrc, "apz_engine.hip"), "-o", out],
                   check=True, stderr=subprocess.DEVNULL)
    return out


def kernels(path):
    """symbol -> (code lines, resource metadata)"""
    lines = open(path).read().split("\n")
    names = [l.split()[1] for l in lines if l.lstrip().startswith(".amdhsa_kernel ")]
    code, cur = {}, None
    for l in lines:
        s = l.split(";")[0].strip()
        if cur is None:
            if s.endswith(":") and s[:-1] in names:
                cur = code.setdefault(s[:-1], [])
        elif s.startswith(".Lfunc_end"):
            cur = None
        elif s and (not s.startswith(".") or s.endswith(":")):      # instructions and labels; no directives
            # .LBB<f>_<b>: f is the function's position in the module, which moves when kernels are added in front of it
            cur.append(LOCAL_LABEL.sub(r".LBB#_\1", s))
    meta, entry = {}, {}
    for l in lines:
        m = re.match(r"^  (- |  )\.(\w+):\s*(\S+)\s*$", l)          # the kernel level of .amdgpu_metadata (arguments sit deeper)
        if not m:
            continue
        if m.group(1) == "- ":
            entry = {}
        entry[m.group(2)] = m.group(3)
        if "name" in entry:
            meta[entry["name"]] = entry
    return {k: (code[k], tuple(meta.get(k, {}).get(f) for f in META)) for k in names}


def verdict(a, b):
    if a is None or b is None:
        return "different"
    (ca, ma), (cb, mb) = a, b
    if ca == cb and ma == mb:
        return "identical"
    ia, ib = ([l for l in c if not l.endswith(":")] for c in (ca, cb))
    hist = lambda ins: collections.Counter(l.split()[0] for l in ins)
    vector = lambda ins: [SGPR.sub("s#", l) for l in ins if not l.startswith("s_")]
    if ma == mb and len(ia) == len(ib) and hist(ia) == hist(ib) and vector(ia) == vector(ib):
        return "scalar-only"
    return "different"


def plain(symbol):
    """mangled symbol -> demangled name without arguments"""
    demangled = subprocess.run(["c++filt", symbol], capture_output=True, text=True).stdout.strip() or symbol
    return demangled.split("(")[0]


def bare(name):
    """... without the return type that a template's name carries"""
    return name[5:] if name.startswith("void ") else name


def main():
    args, renames, keep = [], {}, None
    argv = sys.argv[1:]
    while argv:
        a = argv.pop(0)
        if a == "--keep" and argv:
            keep = argv.pop(0)
        elif a == "--rename" and argv and "=" in argv[0]:
            old, new = argv.pop(0).split("=", 1)
            renames[old] = new
        else:
            args.append(a)
    if len(args) != 2:
        sys.exit(__doc__)
    work = keep or tempfile.mkdtemp(prefix="device_code_diff_")
    os.makedirs(work, exist_ok=True)
    ka, kb = (kernels(assemble(t, os.path.join(work, n))) for t, n in zip(args, ("a.s", "b.s")))
    names = {sym: plain(sym) for sym in set(ka) | set(kb)}
    # A's symbol -> B's symbol: its own, or the one whose name the rename gives
    b_by_name = {bare(names[sym]): sym for sym in kb}
    partner = {sym: b_by_name.get(renames[bare(names[sym])]) for sym in ka if bare(names[sym]) in renames}
    missing = (set(renames) - {bare(names[sym]) for sym in partner}) | {renames[bare(names[s])] for s, t in partner.items() if not t}
    if missing:
        sys.exit("--rename: no such kernel: %s" % ", ".join(sorted(missing)))
    count = collections.Counter()
    for sym in sorted((set(ka) | set(kb)) - set(partner.values())):
        v = verdict(ka.get(sym), kb.get(partner.get(sym, sym)))
        count[v] += 1
        print("%-12s %s" % (v, names[sym] + (" -> " + names[partner[sym]] if sym in partner else "")))
    print("kernels: %d in A, %d in B; " % (len(ka), len(kb)) + ", ".join("%d %s" % (n, v) for v, n in sorted(count.items())))
    sys.exit(1 if count["different"] else 0)


if __name__ == "__main__":
    main()
