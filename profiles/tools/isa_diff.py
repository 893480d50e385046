#!/usr/bin/env python3
"""Device ISA of the floating-point kernels at a git revision against the working tree (no GPU needed):
    profiles/tools/isa_diff.py [REV=HEAD] [-j JOBS]
Compiles, for each tree, every kernels_*.hip that tree has, in both floating-point builds (kernels_fp.hip once per equation
set), with the library's flags plus --cuda-device-only -S (as probe_regs.sh does).  The functions and kernel descriptors
of each build are pooled and matched by demangled name -- a kernel may have moved to another file; those of an anonymous
namespace then change their mangled name -- and compared with labels and symbol names stripped.  Exit status 1 if any
function differs.
--abi: the C-ABI layer instead, every pion_*.hip each tree has, pooled and compared the same way.
--map REGEX=REPL (repeatable): a kernel that was renamed -- the demangled names of REV are rewritten by re.sub before the
match, so that the pair is compared instead of listed as "only in tree" / "only in base", e.g.
    --map 'k_dt_mp\(pion::DtArgs\)=k_dt_mp<0>(pion::DtArgs, pion::CoolForm)' --map 'k_dt_mp_form=k_dt_mp'
-v: for every pair that differs, the instruction counts, the compiler's resource summary (registers, scratch, LDS,
occupancy) of both sides and the differing lines.  --show REGEX: the summary of the matching kernels that are identical, too."""
import argparse
import difflib
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


INFO = {}   # mangled kernel name: resource summary


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
    # the compiler's resource summary of each kernel (comments behind its descriptor): reported by -v, not compared
    for m in re.finditer(r"\.amdhsa_kernel (\S+).*?\.end_amdhsa_kernel(.*?)(?=\.amdhsa_kernel |\Z)", txt, re.S):
        name = m.group(1)
        info = dict(re.findall(r"; (NumVgprs|NumAgprs|TotalNumSgprs|ScratchSize|Occupancy|LDSByteSize|codeLenInByte)\W+(\d+)",
                               m.group(2)))
        INFO[name] = " ".join("%s=%s" % kv for kv in sorted(info.items()))
    return out


def units(tree, abi):
    """[(build, source, flags)] of one tree"""
    csrc = os.path.join(tree, "pion_amd", "csrc")
    if abi:
        return [("abi", src, []) for src in sorted(glob.glob(os.path.join(csrc, "pion_*.hip")))]
    out = []
    for src in sorted(glob.glob(os.path.join(csrc, "kernels_*.hip"))):
        eqs = [[]]
        if os.path.basename(src) == "kernels_fp.hip":
            # (a tree without kernels_prepass.hip is the old layout: PION_EQSEL=0 held the shared kernels)
            old = not os.path.exists(os.path.join(csrc, "kernels_prepass.hip"))
            eqs = [["-DPION_EQSEL=%d" % e] for e in range(0 if old else 1, 4)]
        out += [(mode, src, flags + eq) for mode, flags in MODES.items() for eq in eqs]
    return out


def pooled(trees, abi, tmp, jobs_n):
    """{tag: {build/demangled name: body or descriptor}}, and the sources of each tree"""
    jobs, outs, srcs = [], {}, {}
    for tag, tree in trees:
        for n, (build, src, flags) in enumerate(units(tree, abi)):
            out = os.path.join(tmp, "%s_%d.s" % (tag, n))
            outs.setdefault((tag, build), []).append(out)
            srcs.setdefault(tag, set()).add(os.path.basename(src))
            jobs.append([HIPCC] + COMMON + flags + [src, "-o", out])
    with ThreadPoolExecutor(jobs_n) as ex:
        if any(ex.map(lambda c: subprocess.run(c).returncode, jobs)):
            sys.exit("compile failed")
    pool = {}
    for (tag, build), files in outs.items():
        fns, n = {}, 0
        for f in files:
            one = functions(f)
            n += len(one)
            fns.update(one)
        assert len(fns) == n, "one symbol in two objects"
        names = sorted(fns)
        plain = subprocess.run(["c++filt"], input="\n".join(n.split("#")[0] for n in names), capture_output=True,
                               text=True, check=True).stdout.split("\n")
        mine = {build + "/" + d + ("#descriptor" if n.endswith("#descriptor") else ""): fns[n]
                for n, d in zip(names, plain)}
        assert len(mine) == len(names), "two functions of one demangled name"
        for n, d in zip(names, plain):
            if n in INFO:
                INFO[tag + ":" + build + "/" + d] = INFO[n]
        pool.setdefault(tag, {}).update(mine)
    return pool, {tag: sorted(s) for tag, s in srcs.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("rev", nargs="?", default="HEAD")
    ap.add_argument("-j", type=int, default=8)
    ap.add_argument("--abi", action="store_true")
    ap.add_argument("--map", action="append", default=[], metavar="REGEX=REPL")
    ap.add_argument("-v", action="store_true")
    ap.add_argument("--show", metavar="REGEX")
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        base = os.path.join(tmp, "base")
        os.makedirs(base)
        tar = subprocess.check_output(["git", "-C", HERE, "archive", args.rev, "pion_amd/csrc", "include"])
        subprocess.run(["tar", "-x", "-C", base], input=tar, check=True)
        pool, srcs = pooled((("base", base), ("tree", HERE)), args.abi, tmp, args.j)
    a, b = pool["base"], pool["tree"]
    old = {}   # name after the map: name in REV
    for k in list(a):
        new = k
        for m in args.map:
            new = re.sub(*m.split("=", 1), new)
        assert new == k or new not in a, "--map sends two functions to %s" % new
        old[new] = k
        a[new] = a.pop(k)
    names = sorted(set(a) | set(b))
    diff = [k for k in names if a.get(k) != b.get(k)]
    rows2 = sum("k_stage_rows2" in k and not k.endswith("#descriptor") for k in names)
    print("%s%s -> %s: functions and descriptors compared: %d%s, different: %d" % (
        "C-ABI layer, " if args.abi else "", srcs["base"], srcs["tree"], len(names),
        "" if args.abi else " (k_stage_rows2 instances: %d)" % rows2, len(diff)))
    for k in names if args.show else []:
        if k not in diff and "tree:" + k in INFO and re.search(args.show, k):
            print("SAME", k, "\n  base: %s\n  both: %d lines  %s" % (old[k], len(b[k]), INFO["tree:" + k]))
    for d in diff:
        print("DIFF", d, "(only in %s)" % ("tree" if d not in a else "base") if (d in a) != (d in b) else "")
        if args.v and d in a and d in b:
            print("  base: %s, %d lines  %s" % (old[d], len(a[d]), INFO.get("base:" + old[d], "")))
            print("  tree: %d lines  %s" % (len(b[d]), INFO.get("tree:" + d, "")))
            for line in difflib.unified_diff(a[d], b[d], "base", "tree", n=0, lineterm=""):
                print("    " + line)
    return 1 if diff else 0


if __name__ == "__main__":
    sys.exit(main())
