#!/usr/bin/env python3
"""Time of one pion_gpu_raytrace per source and kernel (profiles/raytrace_timing.json):
    profiles/tools/raytrace_timing.py [--grids 256,512] [--runs 5] [--out profiles/raytrace_timing.json]
    profiles/tools/raytrace_timing.py --once tiles centre 512     (one trace and nothing else: for a kernel trace)
Grids: n^3 Euler with one tracer.  Sources: at the centre vertex, at the low corner, at infinity beyond XN (rays along
x) and beyond ZN (along z); opacity TRACER, so that rho and the tracer are both read.  Kernels: tiles (the default) and
levels (PION_RT_KERNEL=levels); a source at infinity runs the same kernel under either name and is timed once.
Each figure is taken `--runs` times, every run on a fresh handle with a fresh random state (made on the device and
bound to the handle): one untimed trace, then one trace between two HIP events on the handle's stream.  The launches
are pion_gpu_rt_plan's; a kernel trace of `--once` counts them on the device.  Prints one JSON line and, with --out,
writes it there."""
import argparse
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, HERE)

PARENT_STEP_512_MS = (21.0, 21.7)   # README.md: the 512^3 step of the commit before the tracer


def source(cfg, which):
    from pion_amd import abi
    n = cfg.ng[0]
    mid = cfg.xmin[0] + (n // 2) * cfg.dx
    return {
        "centre": {"pos": (mid, mid, mid), "opacity": abi.RT_OPACITY_TRACER},
        "corner": {"pos": (cfg.xmin[0], cfg.xmin[1], cfg.xmin[2]), "opacity": abi.RT_OPACITY_TRACER},
        "infinity_x": {"at_infinity": 1, "dir": 0, "opacity": abi.RT_OPACITY_TRACER},
        "infinity_z": {"at_infinity": 1, "dir": 4, "opacity": abi.RT_OPACITY_TRACER},
    }[which]


def one_run(n, kernel, which, timed=True, check=False):
    """milliseconds of one trace on a fresh handle (None when not timed); check: the columns are read back and looked at"""
    import torch
    from pion_amd import abi, lib
    os.environ["PION_RT_KERNEL"] = kernel
    cfg = abi.make_config(3, [n, n, n], abi.EQEUL, abi.FLUX_RSroe, ntracer=1, dx=1.0 / n, strict_fp=0,
                          bcs=["outflow"] * 6)
    with lib.GpuSim(cfg, 0) as g:
        stream = torch.cuda.current_stream()
        g.set_stream(stream.cuda_stream)
        st = torch.rand(cfg.nvar * g.ncell, dtype=torch.float64, device="cuda:0") + 0.5
        g.bind_device_state(st.data_ptr(), st.data_ptr())
        g.add_rt_source(source(cfg, which))
        if not timed:
            g.raytrace(0)
            g.synchronize()
            return None
        g.raytrace(0)
        g.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        g.raytrace(0)
        e1.record(stream)
        e1.synchronize()
        ms = e0.elapsed_time(e1)
        if check:
            col = g.rt_columns(0, 0)
            assert col.min() >= 0.0 and col.max() > 0.0 and bool((col == col).all())
        del st
        return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grids", default="256,512")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--once", nargs=3, metavar=("KERNEL", "SOURCE", "N"), default=None)
    a = ap.parse_args()
    if a.once:
        one_run(int(a.once[2]), a.once[0], a.once[1], timed=False)
        return
    from pion_amd import abi, lib
    res = {"gpu_lib": os.environ.get("PION_GPU_LIB", "in-tree"), "runs": a.runs, "grids": {}}
    for n in (int(x) for x in a.grids.split(",")):
        cfg = abi.make_config(3, [n, n, n], abi.EQEUL, abi.FLUX_RSroe, ntracer=1, dx=1.0 / n, bcs=["outflow"] * 6)
        grid = {}
        for which in ("centre", "corner", "infinity_x", "infinity_z"):
            tile, launches, levels = lib.rt_plan(cfg, source(cfg, which))
            entry = {"tile": list(tile), "launches_tiles": launches, "launches_levels": levels}
            for kernel in (("tiles", "levels") if which in ("centre", "corner") else ("parallel",)):
                ms = [one_run(n, kernel, which, check=(i == 0)) for i in range(a.runs)]
                entry[kernel] = {"ms": ms, "median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}
            if "levels" in entry:
                entry["tiles_over_levels"] = entry["tiles"]["median_ms"] / entry["levels"]["median_ms"]
                # faster beyond the spread of the runs: every tiles run below every levels run
                entry["tiles_faster_beyond_spread"] = entry["tiles"]["max_ms"] < entry["levels"]["min_ms"]
            if n == 512:
                k = "tiles" if "tiles" in entry else "parallel"
                entry["share_of_parent_step"] = [entry[k]["median_ms"] / t for t in PARENT_STEP_512_MS[::-1]]
            grid[which] = entry
        res["grids"][str(n)] = grid
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
