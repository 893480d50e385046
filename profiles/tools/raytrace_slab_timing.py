#!/usr/bin/env python3
"""Time of pion_gpu_raytrace_part on the slabs of a decomposed domain (profiles/raytrace_slab_timing.json):
    profiles/tools/raytrace_slab_timing.py [--n 512] [--world 8] [--runs 5] [--out profiles/raytrace_slab_timing.json]
The domain is n^3 Euler with one tracer, cut into `world` slabs of n x n x n/world; the sources are raytrace_timing.py's
centre and corner (opacity TRACER), given in the coordinates of the whole domain.  Per source and rank: the role
(pion_gpu_rt_chain), the launches and the workgroups of one launch with the tiles counted from the rank's nearest cell
and, for comparison, from the source vertex (pion_gpu_rt_plan_part), and the time of one pion_gpu_raytrace_part --
the plane received copied in, the trace, both own planes copied out -- `--runs` times, every run on a fresh handle of
that slab with a fresh random state and a random received plane (the time does not depend on the values): one untimed
trace, then one between two HIP events on the handle's stream.  All slabs are timed on ONE device, one after the other.
The chain is serial from the source outwards: chain_ms sums the medians along the longest chain (the transport's own
time is not in it).  Prints one JSON line and, with --out, writes it there."""
import argparse
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, HERE)


def global_cfg(n):
    from pion_amd import abi
    return abi.make_config(3, [n, n, n], abi.EQEUL, abi.FLUX_RSroe, ntracer=1, dx=1.0 / n, strict_fp=0, bcs=["outflow"] * 6)


def source(cfg, which):
    from pion_amd import abi
    mid = cfg.xmin[0] + (cfg.ng[0] // 2) * cfg.dx
    return {"centre": {"pos": (mid, mid, mid), "opacity": abi.RT_OPACITY_TRACER},
            "corner": {"pos": (cfg.xmin[0], cfg.xmin[1], cfg.xmin[2]), "opacity": abi.RT_OPACITY_TRACER}}[which]


def one_run(cfg, part, src, role):
    """milliseconds of one pion_gpu_raytrace_part on a fresh handle"""
    import torch
    from pion_amd import abi, lib
    with lib.GpuSim(cfg, 0) as g:
        stream = torch.cuda.current_stream()
        g.set_stream(stream.cuda_stream)
        st = torch.rand(cfg.nvar * g.ncell, dtype=torch.float64, device="cuda:0") + 0.5
        g.bind_device_state(st.data_ptr(), st.data_ptr())
        g.add_rt_source(src, part=part)
        n = g.rt_count(1)
        fin, lo, hi = (torch.rand(n, dtype=torch.float64, device="cuda:0") for _ in range(3))
        args = (0, 0, fin.data_ptr() if role[0] != abi.RT_RECV_NONE else None, lo.data_ptr() if role[1] else None,
                hi.data_ptr() if role[2] else None)
        g.raytrace_part(*args)
        g.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        g.raytrace_part(*args)
        e1.record(stream)
        e1.synchronize()
        ms = e0.elapsed_time(e1)
        col = g.rt_columns(0, 0)
        assert col.max() > 0.0 and bool((col == col).all())
        del st
        return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--world", type=int, default=8)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from pion_amd import abi, lib, slab
    cfg_g = global_cfg(a.n)
    res = {"n": a.n, "world": a.world, "runs": a.runs, "sources": {}}
    for which in ("centre", "corner"):
        src = source(cfg_g, which)
        ranks = []
        for r in range(a.world):
            cfg = slab.slab_config(cfg_g, r, a.world)
            part = (r * (a.n // a.world), a.n, cfg_g.xmin[2])
            role = lib.rt_chain(cfg, src, part)
            launches, wg, wg0 = lib.rt_plan_part(cfg, src, part)
            ms = [one_run(cfg, part, src, role) for _ in range(a.runs)]
            ranks.append({"rank": r, "recv_side": role[0], "send_lo": role[1], "send_hi": role[2], "launches": launches,
                          "workgroups_per_launch": wg, "workgroups_per_launch_from_vertex": wg0, "ms": ms,
                          "median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)})
        owner = [k["rank"] for k in ranks if k["recv_side"] == abi.RT_RECV_NONE][0]
        up = sum(k["median_ms"] for k in ranks if k["rank"] >= owner)
        down = sum(k["median_ms"] for k in ranks if k["rank"] <= owner)
        res["sources"][which] = {"ranks": ranks, "owner": owner, "chain_ms": max(up, down),
                                 "sum_of_ranks_ms": sum(k["median_ms"] for k in ranks)}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
