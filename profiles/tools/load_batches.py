#!/usr/bin/env python3
"""How the tasks of k_stage_rows2 request their data, read from the ISA (no GPU needed):
    profiles/tools/load_batches.py [REV]      (REV: a git revision instead of the working tree)
Compiles kernels_fp.hip with the compile line of probe_regs.sh (fast build, -DPION_PROBE: the production instances) for
PION_EQSEL 1, 2 and 3 and prints, for every k_stage_rows2 instance, its VGPRs and scratch bytes and, for every copy of
the flux body, what stands ahead of it:
  loads    the global loads requested ahead of the copy
  batches  the runs of global loads that a wait reaching vmcnt(0) separates: 1 = the task pays the way to memory once
  waits    the counts of the waits between the last load and the copy, first..last.  A last count above 0 means that
           the solve starts with that many requests still outstanding (the x task's start-of-step state)
The tool looks at three things only: lines that begin with global_load, lines that begin with s_waitcnt and carry a
vmcnt, and the kernel descriptors.  Every other instruction is a line that is counted and not read.  A copy of the flux
body is one of the longest stretches of the kernel without a load or a wait: three per instance, two in the CYL
instances (x and y), in the order of the kernel's layout.  "(x)" marks a copy with non-temporal loads ahead of it: the
x task of a plain second-order instance, which requests the start-of-step state.  Which of the others is the y task
shows in what stands ahead of them: in the MHD instances the y task has 27 (ideal) or 31 (GLM) loads, the z task 19 or
22 where the z slope is carried in LDS (ZSL).  What stands ahead of a copy ends at the first stretch of more than GAP
instructions without a load or a wait, going back from the copy.  First-order instances prefetch across the solve: no
waits.
Where the listing cannot be trusted: the Euler instances' flux body is a few hundred instructions, no longer than
stretches of the cell update (which also reads the start-of-step state with non-temporal loads), and the listing then
shows such a stretch in place of a copy; an instance that spills reloads from scratch inside the flux body, which cuts
the copy in two at the reload's wait (the cylindrical MHD instances)."""
import os
import re
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
# (the compile line of probe_regs.sh)
FLAGS = ["--offload-arch=gfx950", "-fno-slp-vectorize", "-fPIC", "-std=c++17", "-O2", "-ffp-contract=fast", "-fapprox-func",
         "-freciprocal-math", "-DPION_FAST_MATH", "-DPION_FPNS=fp_fast", "-DPION_PROBE", "--cuda-device-only", "-S", "-w"]
GAP = 120


def events(lines):
    """[(instruction number, 'L' or wait count)] of one kernel, and its instruction count"""
    ev, n = [], 0
    for line in lines:
        s = line.split(";")[0].strip()
        if not s or s.startswith(".") or s.endswith(":"):
            continue
        n += 1
        if s.startswith("global_load"):
            ev.append((n, "N" if s.endswith(" nt") else "L"))   # (N: a non-temporal load)
        elif s.startswith("s_waitcnt"):
            m = re.search(r"vmcnt\((\d+)\)", s)
            if m:
                ev.append((n, int(m.group(1))))
    return ev, n


def copies(ev, n, ncopies):
    """the flux-body copies: [(first instruction, loads, batches, waits)]"""
    pos = [0] + [p for p, _ in ev] + [n]
    # (not the stretch ahead of the first load: the decode of the workgroup's tile)
    gaps = sorted(((pos[i + 1] - pos[i], i) for i in range(1, len(pos) - 1)), reverse=True)[:ncopies]
    out = []
    for length, i in sorted(gaps, key=lambda g: g[1]):
        # what stands ahead: events pos[1..i] = ev[0..i-1], going back until a stretch of more than GAP
        j = i
        while j > 1 and pos[j] - pos[j - 1] <= GAP:
            j -= 1
        ahead = [k for _, k in ev[j - 1:i]]
        once = "N" in ahead
        ahead = ["L" if k == "N" else k for k in ahead]
        while ahead and ahead[0] != "L":
            ahead.pop(0)          # waits for what was requested further back
        loads = ahead.count("L")
        batches, open_run = 0, False
        for k in ahead:
            if k == "L":
                if not open_run:
                    batches += 1
                open_run = True
            elif k == 0:
                open_run = False
        waits = []
        for k in reversed(ahead):
            if k == "L":
                break
            waits.insert(0, k)
        out.append((pos[i], length, loads, batches, waits, once))
    return out


def describe(name):
    m = re.search(r"k_stage_rows2ILi(\d)ELi(\d)ELi(\d+)ELi(\d)ELb(\d)ELb(\d)ELb(\d)E", name)
    eq, ntr, solver, oa, plain, zsl, cyl = (int(x) for x in m.groups())
    return "<EQ %d, NTR %d, solver %d, OAMODE %d, %s%s%s>" % (eq, ntr, solver, oa, "PLAIN" if plain else "general",
                                                             ", ZSL" if zsl else "", ", CYL" if cyl else ""), bool(cyl)


def report(tree):
    src = os.path.join(tree, "pion_amd", "csrc", "kernels_fp.hip")
    with tempfile.TemporaryDirectory() as tmp:
        for eq in (1, 2, 3):
            out = os.path.join(tmp, "probe%d.s" % eq)
            subprocess.run([HIPCC] + FLAGS + ["-DPION_EQSEL=%d" % eq, src, "-o", out], check=True)
            txt = open(out).read()
            for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", txt, re.S):
                name, desc = m.group(1), m.group(2)
                if "k_stage_rows2" not in name:
                    continue
                get = lambda k: re.search(r"\.amdhsa_" + k + r"\s+(\S+)", desc).group(1)
                i0 = txt.index("\n" + name + ":")
                body = txt[i0 + len(name) + 2:txt.index(".Lfunc_end", i0)].split("\n")
                ev, n = events(body)
                what, cyl = describe(name)
                print("PION_EQSEL=%d %s: %s VGPRs, %s bytes of scratch, %d instructions" % (
                    eq, what, get("next_free_vgpr"), get("private_segment_fixed_size"), n))
                for c, (at, length, loads, batches, waits, once) in enumerate(copies(ev, n, 2 if cyl else 3)):
                    w = "none" if not waits else ("%d" % waits[0] if len(waits) == 1 else "%d..%d" % (waits[0], waits[-1]))
                    print("    copy %d%s at %5d (%4d long): %2d loads in %d batch%s, waits %s" % (
                        c + 1, " (x)" if once else "    ", at, length, loads, batches, "" if batches == 1 else "es", w))


def main():
    if len(sys.argv) > 1:
        with tempfile.TemporaryDirectory() as base:
            tar = subprocess.check_output(["git", "-C", HERE, "archive", sys.argv[1], "pion_amd/csrc", "include"])
            subprocess.run(["tar", "-x", "-C", base], input=tar, check=True)
            print("==== %s" % sys.argv[1])
            report(base)
    else:
        print("==== working tree")
        report(HERE)


if __name__ == "__main__":
    main()
