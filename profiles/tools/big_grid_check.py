#!/usr/bin/env python
"""One run of the rows kernel on a grid over 2^29 cells, at its real size.  Opt-in, not a test and not a gate:

    python profiles/tools/big_grid_check.py [--ng 1020 724 724] [--out profiles/rows_windows_big_grid.json]

Euler Roe-CV octant blast (bench.py's M2 set-up) on 1020 x 724 x 724 cells: 1024 x 728 x 728 = 5.43e8 cells per
variable with ghosts, just over the 2^29 one launch of k_stage_rows2 reaches, 2 x 21.7 GB on the device.  Strict
build.  Two steps on the rows kernel in plane windows, then the same two steps with PION_STAGE_KERNEL=cell in a fresh
handle; each in a child process of its own under its own time limit, the second only if the first ended well.  Each
child leaves a digest of P: a BLAKE2 hash of the whole array (equal hashes = equal arrays, without holding two of them
on the host), per-variable sum / min / max and a seeded sample of cells.  The parent compares the digests and writes
agreement and the two throughputs (second step: the first one loads the code objects) to --out.

Before anything it checks the free device memory and the host's MemAvailable; if either is short it writes
"not run: <reason>" and exits 0."""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def _case(ng):
    from pion_amd import abi, problems
    cfg, _ = problems.hd_blast_octant(4, 3, solver=abi.FLUX_RSroe, strict_fp=1)
    L = cfg.dx * 4
    for a in range(3):
        cfg.ng[a] = ng[a]
    cfg.dx = L / ng[0]
    return cfg, problems.fill_hd_blast_octant(cfg, ng[0] / 32.0)


def child(kind, ng, out):
    import numpy as np
    from pion_amd import driver, lib
    if kind == "cell":
        os.environ["PION_STAGE_KERNEL"] = "cell"
    cfg, P = _case(ng)
    res = {"kind": kind, "ng": ng}
    with lib.GpuSim(cfg, 0) as g:
        res["rows_windows"] = g.rows_windows()
        sc = driver.SimControl(g, cfg)
        sc.init(P)
        del P
        ms = []
        for _ in range(2):
            g.synchronize()
            t0 = time.perf_counter()
            sc.calculate_timestep()
            sc.advance_time()
            g.synchronize()
            ms.append(1e3 * (time.perf_counter() - t0))
        res["dt"] = sc.last_dt
        res["ms_per_step"] = ms
        res["mcell_updates_per_s"] = ng[0] * ng[1] * ng[2] / ms[1] / 1e3
        A = g.download(0)
    flat = A.reshape(cfg.nvar, -1)
    res["blake2b"] = hashlib.blake2b(memoryview(A.reshape(-1)).cast("B")).hexdigest()
    res["sum"] = [float(v.sum()) for v in flat]
    res["min"] = [float(v.min()) for v in flat]
    res["max"] = [float(v.max()) for v in flat]
    idx = np.random.default_rng(20261018).integers(0, flat.shape[1], 1 << 20)
    res["sample_blake2b"] = hashlib.blake2b(np.ascontiguousarray(flat[:, idx]).tobytes()).hexdigest()
    res["finite"] = bool(np.isfinite(flat[:, idx]).all())
    with open(out, "w") as f:
        json.dump(res, f)


def _mem_available_gb():
    with open("/proc/meminfo") as f:
        for ln in f:
            if ln.startswith("MemAvailable:"):
                return int(ln.split()[1]) / 1048576.0
    return 0.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ng", type=int, nargs=3, default=[1020, 724, 724])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rows_windows_big_grid.json"))
    ap.add_argument("--child", choices=["rows", "cell"])
    ap.add_argument("--child-out")
    ap.add_argument("--limit-s", type=int, default=420, help="time limit of each child")
    a = ap.parse_args()
    if a.child:
        child(a.child, a.ng, a.child_out)
        return 0

    ncell = (a.ng[0] + 4) * (a.ng[1] + 4) * (a.ng[2] + 4)
    arr_gb = 5 * 8 * ncell / 2.0 ** 30
    need_dev, need_host = 2 * arr_gb + 0.02 * arr_gb * 8 + 2.0, 2.2 * arr_gb + 4.0   # (host: P, the read-back, the flags)
    out = {"ng": a.ng, "cells_per_variable": ncell, "over_the_limit": ncell >= 1 << 29}
    reason = None
    try:
        import torch
        free_dev = torch.cuda.mem_get_info(0)[0] / 2.0 ** 30 if torch.cuda.is_available() else 0.0
    except ImportError:
        free_dev = 0.0
    free_host = _mem_available_gb()
    if free_dev < need_dev:
        reason = "device memory: %.0f GB free, %.0f GB needed" % (free_dev, need_dev)
    elif free_host < need_host:
        reason = "host memory: %.0f GB available, %.0f GB needed" % (free_host, need_host)
    if reason is None:
        tmp = {k: a.out + "." + k for k in ("rows", "cell")}
        for kind in ("rows", "cell"):   # (the second only behind a clean first)
            cmd = ["timeout", "-k", "10", str(a.limit_s), sys.executable, os.path.abspath(__file__), "--child", kind,
                   "--child-out", tmp[kind], "--ng"] + [str(n) for n in a.ng]
            rc = subprocess.call(cmd)
            if rc != 0:
                reason = "the %s run ended with status %d" % (kind, rc)
                break
            with open(tmp[kind]) as f:
                out[kind] = json.load(f)
            os.remove(tmp[kind])
    if reason is not None:
        out["outcome"] = "not run: " + reason
        print(out["outcome"])
    else:
        r, c = out["rows"], out["cell"]
        out["agree"] = all(r[k] == c[k] for k in ("blake2b", "sample_blake2b", "sum", "min", "max", "dt"))
        out["outcome"] = "P after two steps is %s on the windowed rows kernel (%d windows) and on the cell kernel" % (
            "bit-identical" if out["agree"] else "NOT identical", r["rows_windows"]["windows_whole_stage"])
        out["speedup_rows_over_cell"] = r["mcell_updates_per_s"] / c["mcell_updates_per_s"]
        print(out["outcome"])
        print("rows %.0f, cell %.0f Mcell-updates/s" % (r["mcell_updates_per_s"], c["mcell_updates_per_s"]))
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
