#!/usr/bin/env python3
"""Cost of a restart from a FITS file against a restart from the PIONRAW2 file of the same state, and of k_unpack_fits
over a whole grid (profiles/fits_restart.json):
    profiles/tools/fits_restart_cost.py [--n 256] [--dir /dev/shm] [--reps 5] [--only pionraw]
One GLM-MHD state of n^3 cells (fast build) is written once to both files under --dir (a tmpfs path), then each restart
is timed --reps times after one warm-up, from the call to a synchronised device.  --only pionraw: the PIONRAW2 restart
alone, for libraries that predate the FITS reader (PION_GPU_LIB / PION_HOST_LIB name them).  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, HERE)


def timed(fn, sync, reps):
    fn()
    sync()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        sync()
        out.append(time.perf_counter() - t0)
    return {"median_s": statistics.median(out), "min_s": min(out), "max_s": max(out), "runs": out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--dir", default="/dev/shm")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", choices=["pionraw"], default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    from pion_amd import host_rccl, lib, problems
    cfg, P = problems.mhd_blast_generic([a.n] * 3, strict_fp=0)
    raw, fits = os.path.join(a.dir, "fits_restart_cost.pionraw"), os.path.join(a.dir, "fits_restart_cost.fits")
    res = {"n": a.n, "nvar": cfg.nvar, "gpu_lib": os.environ.get("PION_GPU_LIB", "in-tree"),
           "host_lib": os.environ.get("PION_HOST_LIB", "in-tree")}
    try:
        with host_rccl.HostSim(cfg, 0) as s:
            s.init(P)
            del P
            g = lib.GpuSim(cfg, 0, borrowed_handle=s.gpu_handle())
            s.write_snapshot(raw)
            res["pionraw_bytes"] = os.path.getsize(raw)
            res["restart_pionraw"] = timed(lambda: s.restart(raw), g.synchronize, a.reps)
            if a.only is None:
                s.write_fits(fits)
                res["fits_bytes"] = os.path.getsize(fits)
                res["restart_fits"] = timed(lambda: s.restart(fits), g.synchronize, a.reps)
                nplanes = cfg.ng[2]
                n = g.fits_prim_count(nplanes)
                buf = torch.from_numpy(np.random.default_rng(3).uniform(0.5, 1.5, size=n).astype(">f8").view("=f8")).to("cuda:0")
                torch.cuda.synchronize()
                k = timed(lambda: g.unpack_fits(0, nplanes, buf.data_ptr()), g.synchronize, 20)
                assert g.unpack_fits_status() == 0
                k["bytes_moved"] = 3 * 8 * n   # the buffer read, P and Ph written
                k["GB_per_s_median"] = k["bytes_moved"] / k["median_s"] / 1e9
                k["GB_per_s_best"] = k["bytes_moved"] / k["min_s"] / 1e9
                k.pop("runs")
                res["k_unpack_fits_whole_grid"] = k
    finally:
        for f in (raw, fits):
            if os.path.exists(f):
                os.unlink(f)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
