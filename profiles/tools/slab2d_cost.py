"""Cost of the 2-D row-range launches on one GPU: one rank's slab of the MHD2D and MHDAXI2D workloads at world 8
(4096 x 768 and 4096 x 256), fast build.

  (a) whole : every stage as one whole-stage launch (pion_gpu_stage)
  (b) split : every stage as PION_STAGE_INTERIOR + PION_STAGE_SLABBOUNDARY on the compute stream (no communication
              stream: the two launches run one after the other, so (b) is the sum of their costs)

What is timed: the stage calls only (prepass, cooling source, stage kernel[s] of the half step and of the full step), by
HIP events on the compute stream, summed per step; the boundary update, the time step and the refill of the slab's halo
rows (device copies through pion_gpu_halo_spans: the slab is its own neighbour) lie outside the event pairs.
Per mode: RUNS runs of STEPS steps after WARMUP steps; reported: the median over the runs of the per-run mean, min, max.

  python profiles/tools/slab2d_cost.py [--whole-only] [--out FILE]     (PION_GPU_LIB=... for another build of the library;
  a build without 2-D slabs can only run --whole-only)
"""
import argparse
import copy
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from pion_amd import abi, lib, problems  # noqa: E402

STEPS, RUNS, WARMUP = 20, 5, 3


def workload(name):
    if name == "mhd2d":
        cfg, _ = problems.mhd_blastwave(4, 2, abi.EQGLM, abi.FLUX_RS_HLLD, strict_fp=0)
        cfg.ng[0], cfg.ng[1] = 4096, 768
        cfg.dx = 1.0 / 4096
        cfg.xmin[1] = -0.5 * 768 / 4096
        return cfg, problems.fill_mhd_blastwave(cfg)
    cfg, P = problems.blast_axi2d(4096, abi.EQGLM, abi.FLUX_RS_HLLD, strict_fp=0)   # 4096 x 2048: rank 0 of 8
    cfg.ng[1] = 256
    return cfg, P[:, :, :256 + 2 * cfg.nbc].copy()


def _hip():
    """the HIP runtime this process already uses (the one libpion_gpu.so is bound to)"""
    with open("/proc/self/maps") as f:
        paths = sorted({ln.split()[-1] for ln in f if "libamdhip64" in ln})
    h = C.CDLL(paths[0])
    h.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    return h


def refill(g, hip, which, lo_slab, hi_slab, stream):
    """the halo rows of the slab axis from the slab's own rows (not timed)"""
    sp = g.halo_spans(which)
    nb = sp["count_per_var"] * 8
    for v in range(sp["nvar"]):
        o = v * sp["var_stride"] * 8
        if lo_slab:
            hip.hipMemcpyAsync(sp["recv_lo"] + o, sp["send_hi"] + o, nb, 3, stream)
        if hi_slab:
            hip.hipMemcpyAsync(sp["recv_hi"] + o, sp["send_lo" if lo_slab else "send_hi"] + o, nb, 3, stream)


def run(name, split):
    cfg, P = workload(name)
    c = copy.deepcopy(cfg)
    lo_slab = hi_slab = False
    if split:
        hi_slab = True
        lo_slab = cfg.bc_type[2] == abi.BC_PERIODIC      # (the axis stays on the cylindrical slab)
        c.bc_type[3] = abi.BC_SLAB
        if lo_slab:
            c.bc_type[2] = abi.BC_SLAB
    ks = torch.cuda.Stream()
    with lib.GpuSim(c, 0) as g:
        hip = _hip() if split else None
        g.set_stream(ks.cuda_stream)
        g.upload(P)
        t = 0.0
        g.update_bcs(t, 2, 2, assign=1)

        def stage(dt, ooa, full, ev):
            if split:
                refill(g, hip, 0 if ooa == 1 else 1, lo_slab, hi_slab, ks.cuda_stream)
            with torch.cuda.stream(ks):
                ev[0].record()
            if split:
                g.stage_part(dt, ooa, full, abi.STAGE_INTERIOR)
                g.stage_part(dt, ooa, full, abi.STAGE_SLABBOUNDARY)
            else:
                g.stage(dt, ooa, full)
            with torch.cuda.stream(ks):
                ev[1].record()

        def step(evs):
            nonlocal t
            t_dyn, t_mp = g.calc_dt()
            dt = min(t_dyn, t_mp)
            g.set_glm_speeds(t_dyn, c.dx, 0.25 / c.dx)
            stage(0.5 * dt, 1, 0, evs[0])
            g.update_bcs(t, 1, 2)
            stage(dt, 2, 1, evs[1])
            g.update_bcs(t, 2, 2)
            t += dt

        mk = lambda: [[torch.cuda.Event(enable_timing=True) for _ in range(2)] for _ in range(2)]
        for _ in range(WARMUP):
            step(mk())
        means = []
        for _ in range(RUNS):
            evs = [mk() for _ in range(STEPS)]
            for e in evs:
                step(e)
            g.synchronize()
            ks.synchronize()
            means.append(sum(a[0].elapsed_time(a[1]) + b[0].elapsed_time(b[1]) for a, b in evs) / STEPS)
        return {"median_ms_per_step": statistics.median(means), "min": min(means), "max": max(means), "runs": means}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--whole-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"library": os.environ.get("PION_GPU_LIB", "libpion_gpu.so of this tree"), "steps": STEPS, "runs": RUNS,
           "what": "stage calls of one step (half + full stage), HIP events, ms", "workloads": {}}
    for name, shape in (("mhd2d", "4096 x 768"), ("mhdaxi2d", "4096 x 256")):
        w = {"slab": shape, "whole": run(name, False)}
        if not a.whole_only:
            w["interior_plus_strips"] = run(name, True)
        res["workloads"][name] = w
        print(name, json.dumps(w), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
