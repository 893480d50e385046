#!/usr/bin/env python3
"""Device ISA of kernels_fp.hip at a git revision against the working tree, both floating-point builds and every
equation set (no GPU needed):  profiles/tools/isa_diff.py [REV=HEAD] [-j JOBS]
Compiles with the library's flags plus --cuda-device-only -S (as probe_regs.sh does) and compares every function body
and kernel descriptor with labels and symbol names stripped.  Exit status 1 if any function differs.
--abi: the C-ABI layer instead, every pion_*.hip each tree has, its functions pooled and matched by demangled name
(a kernel may have moved to another file; those of an anonymous namespace then change their mangled name)."""
import argparse
import os
import re
import subprocess
import sys
import glob
import tempfile
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
COMMON = ["--offload-arch=gfx950", "-fno-slp-vectorize", "-fPIC", "-std=c++17", "-O2", "-w", "--cuda-device-only", "-S"]
MODES = {"strict": ["-ffp-contract=off", "-DPION_FPNS=fp_strict"],
         "fast": ["-ffp-contract=fast", "-fapprox-func", "-freciprocal-math", "-DPION_FAST_MATH", "-DPION_FPNS=fp_fast"]}


def functions(path):
    txt = open(path).read()
    out = {}
    for name in re.findall(r"\.type\s+(\S+),@function", txt):
        i0 = txt.index("\n" + name + ":")
        i1 = txt.index(".Lfunc_end", i0)
        lines = []
        for line in txt[i0 + len(name) + 2:i1].split("\n"):
            s = line.split(";")[0].strip()
            if not s or (s.startswith(".") and not s.startswith(".LBB")):
                continue
            s = re.sub(r"\.LBB\d+_\d+", "L", s)
            s = re.sub(r"\.Ltmp\d+", "T", s)
            lines.append(re.sub(r"_Z\w+", "SYM", s))
        out[name] = lines
    for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", txt, re.S):
        out[m.group(1) + "#descriptor"] = [l.strip() for l in m.group(2).split("\n") if l.strip()]
    return out


def abi_layer(trees, tmp, jobs_n):
    """{tag: {demangled name: body or descriptor}} over the pion_*.hip of each tree; then the comparison"""
    jobs, outs = [], {}
    for tag, tree in trees:
        for src in sorted(glob.glob(os.path.join(tree, "pion_amd", "csrc", "pion_*.hip"))):
            out = os.path.join(tmp, "%s_%s.s" % (tag, os.path.basename(src)))
            outs.setdefault(tag, []).append(out)
            jobs.append([HIPCC] + COMMON + [src, "-o", out])
    with ThreadPoolExecutor(jobs_n) as ex:
        if any(ex.map(lambda c: subprocess.run(c).returncode, jobs)):
            sys.exit("compile failed")
    pooled = {}
    for tag, files in outs.items():
        fns = {}
        for f in files:
            fns.update(functions(f))
        names = sorted(fns)
        plain = subprocess.run(["c++filt"], input="\n".join(n.split("#")[0] for n in names), capture_output=True,
                               text=True, check=True).stdout.split("\n")
        pooled[tag] = {d + ("#descriptor" if n.endswith("#descriptor") else ""): fns[n] for n, d in zip(names, plain)}
        assert len(pooled[tag]) == len(names), "two functions of one demangled name"
    a, b = pooled["base"], pooled["tree"]
    diff = [k for k in sorted(set(a) | set(b)) if a.get(k) != b.get(k)]
    print("C-ABI layer, %s -> %s: functions and descriptors compared: %d, different: %d" % (
        [os.path.basename(f)[5:-2] for f in outs["base"]], [os.path.basename(f)[5:-2] for f in outs["tree"]],
        len(set(a) | set(b)), len(diff)))
    for d in diff:
        print("DIFF", d, "(only in %s)" % ("tree" if d not in a else "base") if (d in a) != (d in b) else "")
    return 1 if diff else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("rev", nargs="?", default="HEAD")
    ap.add_argument("-j", type=int, default=8)
    ap.add_argument("--abi", action="store_true")
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        base = os.path.join(tmp, "base")
        os.makedirs(base)
        tar = subprocess.check_output(["git", "-C", HERE, "archive", args.rev, "pion_amd/csrc", "include"])
        subprocess.run(["tar", "-x", "-C", base], input=tar, check=True)
        if args.abi:
            return abi_layer((("base", base), ("tree", HERE)), tmp, args.j)
        jobs = []
        for tree, tag in ((base, "base"), (HERE, "tree")):
            for mode, flags in MODES.items():
                for eq in range(4):
                    out = os.path.join(tmp, "%s_%s_%d.s" % (tag, mode, eq))
                    jobs.append([HIPCC] + COMMON + flags + ["-DPION_EQSEL=%d" % eq,
                                                              os.path.join(tree, "pion_amd", "csrc", "kernels_fp.hip"),
                                                              "-o", out])
        with ThreadPoolExecutor(args.j) as ex:
            for rc in ex.map(lambda c: subprocess.run(c).returncode, jobs):
                if rc:
                    sys.exit("compile failed")
        total = rows2 = 0
        diff = []
        for mode in MODES:
            for eq in range(4):
                a = functions(os.path.join(tmp, "base_%s_%d.s" % (mode, eq)))
                b = functions(os.path.join(tmp, "tree_%s_%d.s" % (mode, eq)))
                for k in sorted(set(a) | set(b)):
                    total += 1
                    rows2 += ("k_stage_rows2" in k and not k.endswith("#descriptor"))
                    if a.get(k) != b.get(k):
                        diff.append("%s/%d %s" % (mode, eq, k))
    print("functions and descriptors compared: %d (k_stage_rows2 instances: %d), different: %d" % (total, rows2,
                                                                                                 len(diff)))
    for d in diff:
        print("DIFF", d)
    return 1 if diff else 0


if __name__ == "__main__":
    sys.exit(main())
